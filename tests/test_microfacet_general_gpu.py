"""The general MicrofacetDistribution on the GPU (include/ppg.h ppg_set_microfacet; csrc: the extended kernels, PPG_MFD), through the test hook
ppg_debug_bsdf whose lanes call the render's own mat_eval / mat_pdf / mat_sample:

  * the hook gives the oracle's values bit for bit for today's isotropic materials, and the same materials stated as general entries
    (alpha_v = alpha) give the same bits again — in the hook and in a render through the extended kernels;
  * eval, pdf and the sampled normal of every distribution type, sampler and roughness pair equal the float64 restatement of
    test_microfacet_general.py;
  * the three plug-ins are consistent in themselves (test_bsdfs.py's checks): weight = eval / pdf, the pdf integrates to the probability of
    producing a sample, sampled directions follow it;
  * the host paths: determinism, clearing the list, the refusals.
"""
import os

import numpy as np
import pytest

from conftest import CBOX_PROPS, IMPROVED
from test_bsdfs import GOLD, SMOOTH, bsdf_eval, bsdf_sample, rtrans_slice, sphere_grid, unit
from test_microfacet_general import ALPHAS, CASES, TYPES, WIS, Distribution, _id, conductor_eval_pdf
from test_rfilter_gpu import _hash, _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def path_key(seed, pixel, sample):
    """include/ppg_rng.h ppg_path_key"""
    with np.errstate(over="ignore"):
        k = _hash(np.uint32(seed & 0xffffffff) ^ np.uint32(0x9e3779b9))
        k = _hash(k ^ np.uint32(seed >> 32))
        k = _hash(k + np.asarray(pixel, np.uint32) * np.uint32(0x9e3779b1))
        return _hash(k ^ (np.uint32(sample) * np.uint32(0x85ebca77) + np.uint32(0xc2b2ae3d)))


def phong_slice(alpha, eta):
    g = np.load(os.path.join(GOLDEN, "rtrans_slices_phong.npz"))
    for i, (d, a, e) in enumerate(g["cases"]):
        if (str(d), float(a), float(e)) == ("phong", alpha, eta):
            return g["slice%d" % i]
    raise KeyError((alpha, eta))


def scene_with(materials, width=16, height=12):
    """the Cornell box with `materials` appended to its own (none of them on a triangle); slices of roughplastic ones gathered into rtrans"""
    import ppg_host
    desc = ppg_host.cbox_scene(width, height)
    base = len(desc.materials)
    slices, mats = [], []
    for m in materials:
        m = dict(m)
        if "slice" in m:
            m["rtrans"] = len(slices)
            slices.append(np.asarray(m.pop("slice"), f32))
        mats.append(m)
    desc.materials = list(desc.materials) + mats
    desc.rtrans = np.stack(slices) if slices else None
    return desc, base


def general(m):
    """the same material stated as a general entry"""
    return dict(m, alpha_v=m["alpha"])


ROUGH = [(n, m) for n, m in SMOOTH if n.startswith("ggx")]
N = 4 * 4096


def lattice():
    """the four wi of test_bsdfs.py, 4096 items each; u on a 64 x 64 lattice with u.x in [1e-3, 1 - 1e-3] and u.y (j + 0.5) / 64, at least
    1/128 from every multiple of 1/4; wo on a lattice of the sphere (both hemispheres: the dielectric transmits)"""
    wi = np.repeat(np.stack([unit(w) for w in WIS.values()]), N // 4, 0)
    i, j = np.divmod(np.arange(N // 4), 64)
    ux = (1e-3 + (i + 0.5) / 64 * (1 - 2e-3)).astype(f32)
    uy = ((j + 0.5) / 64).astype(f32)
    u = np.tile(np.stack([ux, uy], 1), (4, 1))
    cz = (((j + 0.5) / 64) * 2 - 1) * 0.97
    cz = np.where(np.abs(cz) < 0.05, 0.05, cz)
    ph = 2 * np.pi * (i + 0.37) / 64
    wo = np.stack([np.sqrt(1 - cz * cz) * np.cos(ph), np.sqrt(1 - cz * cz) * np.sin(ph), cz], 1)
    wo = np.tile(wo / np.linalg.norm(wo, axis=1, keepdims=True), (4, 1)).astype(f32)
    assert np.all(np.abs(wi[:, 2]) >= 0.05) and np.all(np.abs(u[:, 1] * 4 - np.round(u[:, 1] * 4)) >= 4e-3)
    return wi, wo, u


@pytest.fixture(scope="module")
def hook_iso():
    """hook results of test_bsdfs.SMOOTH's rough materials, plain and stated as general entries"""
    desc, base = scene_with([m for _, m in ROUGH] + [general(m) for _, m in ROUGH])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    wi, wo, u = lattice()
    keys = path_key(77, np.arange(N), 0)  # the oracle's sampler for item i (ppgo_bsdf_sample)
    out = [e.debug_bsdf(base + k, wi, wo, u, keys) for k in range(2 * len(ROUGH))]
    e.close()
    return out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("k", range(len(ROUGH)), ids=[n for n, _ in ROUGH])
def test_hook_equals_the_oracle_bit_for_bit(oracle_lib, hook_iso, k):
    mat = ROUGH[k][1]
    wi, wo, u = lattice()
    f, p = bsdf_eval(oracle_lib, mat, wi, wo)
    swo, w, spdf, eta, delta = bsdf_sample(oracle_lib, mat, wi, u)
    g = hook_iso[k]
    assert np.array_equal(bits(g["eval"]), bits(f)) and np.array_equal(bits(g["pdf"]), bits(p))
    assert np.array_equal(bits(g["weight"]), bits(w))
    ok = w.any(1)  # (a failed sample leaves the other fields of the record unspecified)
    assert ok.sum() > N // 4
    for name, ref in (("wo", swo), ("sampled_pdf", spdf), ("eta", eta)):
        assert np.array_equal(bits(g[name][ok]), bits(ref[ok])), name
    assert np.array_equal(g["delta"][ok], delta[ok])


@pytest.mark.parametrize("k", range(len(ROUGH)), ids=[n for n, _ in ROUGH])
def test_general_entry_with_equal_alphas_reduces_to_the_isotropic_path(hook_iso, k):
    a, b = hook_iso[k], hook_iso[len(ROUGH) + k]
    for name in a.dtype.names:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


def _box_scene(as_general):
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    mats = [dict(GOLD, distribution="beckmann"), dict(SMOOTH[8][1]), dict(SMOOTH[11][1])]  # conductor, rough dielectric, two-sided rough plastic
    assert mats[1]["type"] == "roughdielectric" and mats[2]["type"] == "roughplastic"
    mats[2]["rtrans"] = 0
    desc.rtrans = np.asarray(mats[2].pop("slice"), f32)[None]
    if as_general:
        mats = [general(m) for m in mats]
    base = len(desc.materials)
    desc.materials = list(desc.materials) + mats
    tm = np.array(desc.tri_material)
    box = np.nonzero(tm == 0)[0]
    assert len(box) == 24  # the two boxes, six faces each
    tm[box] = base + np.arange(24) * 3 // 24
    desc.tri_material = tm
    return desc


def _box_render(as_general):
    e = hip(**dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=11, nee="always"))
    e.set_scene(_box_scene(as_general))
    e.render()
    out = e.read_film(), e.read_sdtree()
    e.close()
    return out


def test_render_through_the_extended_kernels_equals_todays():
    fa, ta = _box_render(False)
    fb, tb = _box_render(True)
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


# ------------------------------------------------------------------------------------------------ against the restatement
MIRROR = dict(type="roughconductor", eta=(0, 0, 0), k=(1, 1, 1), reflectance=(1, 1, 1), twosided=True)  # Fresnel = 1; two-sided: wi from below counts
COMBOS = [(k, sa, a) for k in TYPES for sa in (False, True) for a in ALPHAS if not (k == "phong" and not sa)]

# Largest angle between the sampled normals — the quantity this test looks at, normalize(wi + wo) with wo the mirror image of wi in the
# sampled normal — of the restatement run in numpy float32 and in float64 over this test's own inputs (all cases), measured on the CPU, and
# the bound derived from it: 8 x, for the dm_* functions of include/ppg_detmath.h differing from numpy's by a few ulp over chains of up to
# six calls.  With all normals sampled, a normal nearly at right angles to a grazing wi leaves wi + wo = 2 (wi . m) m a difference of nearly
# equal float32 vectors, and the rebuilt normal loses digits in proportion: those cases set the largest figures.
NORMAL_ANGLE_F32_VS_F64 = 7.4199e-3  # radians, measured: phong, (0.3, 0.05).  By case: beckmann visible 5.4e-7 .. 8.4e-7, ggx visible 2.9e-5 ..
#                                      8.0e-5, beckmann all 4.9e-5 .. 2.6e-3, ggx all 1.2e-4 .. 9.1e-4, phong 2.2e-4 .. 7.4e-3
NORMAL_ANGLE_BOUND = 8 * NORMAL_ANGLE_F32_VS_F64  # 5.9359e-2
# Each case is held to its own figure: 8 x the angle measured the same way for its type, sampler and roughness pair (over the four wi), never
# below 8 x 2^-23, the spacing of the float32 components the normal is rebuilt from, and never above the bound of all cases.
_case_angle = {}


def case_bound(kind, sample_all, alphas):
    key = (kind, sample_all, alphas)
    if key not in _case_angle:
        wi, _, u = restatement_inputs()
        wi1 = one_sided(wi, wi)
        h = []
        for dt in (np.float32, np.float64):  # the quantity the test looks at, start to end in one precision: m, wo = its mirror image of wi, normalize(wi + wo)
            w = wi1.astype(dt)
            m, _ = Distribution(kind, f32(alphas[0]), f32(alphas[1]), dt).sample(w, u.astype(dt), sample_all)
            wo = dt(2) * (w * m).sum(1, dtype=dt)[:, None] * m - w
            hh = w + wo
            h.append(hh / np.sqrt((hh * hh).sum(1, dtype=dt))[:, None])
        _case_angle[key] = float(angle(h[0], h[1]).max())
    return min(NORMAL_ANGLE_BOUND, 8 * max(_case_angle[key], 2.0 ** -23)), _case_angle[key]


def combo_material(kind, sample_all, alphas):
    m = dict(MIRROR, alpha=alphas[0], alpha_v=alphas[1])
    if kind != "ggx":
        m["distribution"] = kind
    if sample_all:
        m["sample_visible"] = False
    return m


def restatement_inputs():
    """per wi (in test_bsdfs.py's order): wi, wo and u of the lattice above, with wo mirrored into wi's hemisphere"""
    wi, wo, u = lattice()
    wo = wo.copy()
    wo[:, 2] = np.abs(wo[:, 2]) * np.sign(wi[:, 2])
    return wi, wo, u


def one_sided(wi, v):
    """the two-sided adapter's view: the frame in which wi is above the surface"""
    s = np.where(wi[:, 2:3] < 0, -1.0, 1.0)
    return v * np.concatenate([np.ones_like(s), np.ones_like(s), s], 1)


def angle(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


@pytest.fixture(scope="module")
def hook_combos():
    desc, base = scene_with([combo_material(*c) for c in COMBOS])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    wi, wo, u = restatement_inputs()
    out = {c: e.debug_bsdf(base + k, wi, wo, u) for k, c in enumerate(COMBOS)}
    e.close()
    return out


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_distribution_equals_the_restatement(hook_combos, case):
    kind, sample_all, alphas, wname = case
    w = list(WIS).index(wname)
    sl = slice(w * (N // 4), (w + 1) * (N // 4))
    wi, wo, u = (a[sl] for a in restatement_inputs())
    g = hook_combos[(kind, sample_all, alphas)][sl]
    D = Distribution(kind, f32(alphas[0]), f32(alphas[1]))
    wi1, wo1 = one_sided(wi, wi).astype(np.float64), one_sided(wi, wo).astype(np.float64)
    f, p = conductor_eval_pdf(D, sample_all, wi1, wo1)
    print("eval: max rel", np.max(np.abs(g["eval"][:, 0] - f) / np.maximum(np.abs(f), 1e-3)), "pdf: max rel", np.max(np.abs(g["pdf"] - p) / np.maximum(np.abs(p), 1e-3)))
    assert np.allclose(g["eval"][:, 0], f, rtol=2e-3, atol=1e-6) and np.all(g["eval"][:, 0] == g["eval"][:, 1])
    assert np.allclose(g["pdf"], p, rtol=2e-3, atol=1e-6)
    # the sampled normal as the sampled direction shows it: normalize(wi + wo) in the one-sided frame, for the kernel's wo and for the
    # restatement's (the mirror image of wi in its normal; with all normals sampled one may face away from wi, and both sides then see -m).
    # A sample that fails the side check keeps the reflected direction in that frame: the adapter turns only successful ones back.
    m64, pdf64 = D.sample(wi1, u.astype(np.float64), sample_all)
    assert np.all(pdf64 > 0) and np.all(g["sampled_pdf"] > 0)
    refl = 2 * (wi1 * m64).sum(1)[:, None] * m64 - wi1
    h64 = wi1 + refl
    h64 = h64 / np.linalg.norm(h64, axis=1, keepdims=True)
    failed = ~g["weight"].any(1)
    swo = np.where(failed[:, None], g["wo"], one_sided(wi, g["wo"])).astype(np.float64)
    h = wi1 + swo
    m = h / np.linalg.norm(h, axis=1, keepdims=True)
    a = angle(m, h64)
    bound, measured = case_bound(kind, sample_all, alphas)
    print("sampled normal: max angle", a.max(), "float32 vs float64 in this case", measured, "bound", bound)
    assert a.max() <= bound
    # a sample fails exactly where the reflected direction leaves the hemisphere
    sure = np.abs(refl[:, 2]) > 1e-3
    assert np.array_equal(failed[sure], (refl[:, 2] <= 0)[sure])


# ------------------------------------------------------------------------------------------------ the three plug-ins, test_bsdfs.py's checks
PLUGINS = [
    ("conductor-ggx-0.05-0.3", dict(GOLD, alpha=0.05, alpha_v=0.3)),
    ("conductor-phong-0.3-0.1", dict(GOLD, alpha=0.3, alpha_v=0.1, distribution="phong")),
    ("roughdielectric-beckmann-0.1-0.4-all", dict(type="roughdielectric", alpha=0.1, alpha_v=0.4, eta=1.5, reflectance=(1, 1, 1), specular=(0.9, 0.95, 1.0),
                                                   distribution="beckmann", sample_visible=False)),
    ("roughdielectric-ggx-0.3-0.3-all", dict(type="roughdielectric", alpha=0.3, alpha_v=0.3, eta=1.5, reflectance=(1, 1, 1), specular=(0.9, 0.95, 1.0),
                                              sample_visible=False)),
    ("roughplastic-phong-0.2", dict(type="roughplastic", alpha=0.2, eta=1.5, distribution="phong", reflectance=(0.6, 0.3, 0.1), specular=(1, 1, 1),
                                    slice=phong_slice(0.2, 1.5))),
]


@pytest.fixture(scope="module")
def plugin_engine():
    desc, base = scene_with([m for _, m in PLUGINS])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    yield e, base
    e.close()


@pytest.mark.parametrize("k", range(len(PLUGINS)), ids=[n for n, _ in PLUGINS])
@pytest.mark.parametrize("wname", list(WIS))
def test_plugins_sampling_matches_pdf_and_weight_matches_eval(plugin_engine, k, wname):
    """test_bsdfs.py::test_sampling_matches_pdf_and_weight_matches_eval with its tolerances, through the hook.  (2): with sampling of all
    normals the reflected direction of a sampled normal may leave the hemisphere, so the pdf integrates to the fraction of draws that
    produce a sample — the bound is that file's non-ggx one around this fraction."""
    e, base = plugin_engine
    name, mat = PLUGINS[k]
    wi = unit(WIS[wname])
    rng = np.random.RandomState(7)
    xy = rng.rand(400000, 2).astype(f32)
    keys = _hash(np.arange(len(xy), dtype=np.uint32) + np.uint32(12345))
    s = e.debug_bsdf(base + k, wi, np.zeros((len(xy), 3), f32) + f32([0, 0, 1]), xy, keys)
    wo, w, pdf, eta, delta = s["wo"], s["weight"], s["sampled_pdf"], s["eta"], s["delta"]
    ok = (pdf > 0) & (w.sum(1) > 0)
    if wi[2] < 0 and "roughdielectric" not in name:
        assert not ok.any()
        return
    smooth = ok & (delta == 0)
    assert np.all(delta == 0)
    if "roughdielectric" in name:
        trans = ok & (wo[:, 2] * wi[2] < 0)
        e_mat = float(f32(mat["eta"]))
        assert trans.any() and np.allclose(eta[trans], e_mat if wi[2] > 0 else 1 / e_mat, rtol=1e-6) and np.all(eta[ok & ~trans] == 1)
    else:
        assert np.all(eta[ok] == 1)
    # (1)
    q = e.debug_bsdf(base + k, wi, wo[smooth], xy[:1], keys[:1])
    f, p = q["eval"], q["pdf"]
    assert np.all(p > 0)
    assert np.allclose(w[smooth], f / p[:, None], rtol=2e-3, atol=1e-6)
    assert np.allclose(pdf[smooth], p, rtol=2e-3, atol=1e-7)
    # (2)
    d, dw, shape = sphere_grid()
    q = e.debug_bsdf(base + k, wi, d, xy[:1], keys[:1])
    fg, pg = q["eval"], q["pdf"]
    if "roughdielectric" in name:
        pg = np.where(fg.sum(1) > 0, pg, 0).astype(f32)  # test_bsdfs.py:127
    total = float((pg.astype(np.float64) * dw).sum())
    print(name, wname, "integral of the pdf", total, "fraction of draws that give a sample", ok.mean())
    assert abs(total - ok.mean()) < 0.01 and total <= 1.005
    # (3)
    nb_t, nb_p = 18, 12
    H = (pg.astype(np.float64) * dw).reshape(shape).reshape(nb_t, shape[0] // nb_t, nb_p, shape[1] // nb_p).sum((1, 3))
    ws = wo[smooth].astype(np.float64)
    it = np.clip((np.arccos(np.clip(ws[:, 2], -1, 1)) / np.pi * nb_t).astype(int), 0, nb_t - 1)
    ip = np.clip(((np.arctan2(ws[:, 1], ws[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nb_p).astype(int), 0, nb_p - 1)
    cnt = np.zeros((nb_t, nb_p)); np.add.at(cnt, (it, ip), 1)
    emp = cnt / len(xy)
    big = H > 2e-3
    assert big.sum() >= 3
    assert np.allclose(emp[big], H[big], rtol=0.08, atol=2e-4), (np.abs(emp[big] / H[big] - 1).max())


# ------------------------------------------------------------------------------------------------ renders
def _plate_scene(material, turned=False):
    """the 64 x 48 Cornell box with a tilted two-triangle plate that carries texture coordinates; `turned`: its texture coordinates turned
    by 90 degrees, (u, v) -> (v, 1 - u), so that dpdu points where dpdv did"""
    import ppg_host
    d = ppg_host.cbox_scene(64, 48)
    n = unit((0.1, 0.8, -0.6)).astype(np.float64)
    a = np.cross(n, (0.0, 0.0, 1.0)); a = 150 * a / np.linalg.norm(a)
    b = np.cross(n, a); b = 110 * b / np.linalg.norm(b)  # a, b, n orthogonal: the UV tangents are the frame's own axes either way
    c = np.array([278.0, 230.0, 300.0])
    quad = np.stack([c - a - b, c + a - b, c + a + b, c - a + b]).astype(f32)
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], f32)
    if turned:
        uv = np.stack([uv[:, 1], 1 - uv[:, 0]], 1).astype(f32)
    nv = len(d.positions)
    d.positions = np.concatenate([np.asarray(d.positions, f32), quad])
    d.indices = np.concatenate([np.asarray(d.indices, np.uint32), np.array([[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]], np.uint32)])
    d.materials = list(d.materials) + [material]
    d.tri_material = np.concatenate([np.asarray(d.tri_material, np.uint32), np.full(2, len(d.materials) - 1, np.uint32)])
    d.tri_emitter = np.concatenate([np.asarray(d.tri_emitter, np.int32), np.full(2, -1, np.int32)])
    assert d.normals is None
    d.texcoords = np.concatenate([np.full((nv, 2), np.nan, f32), uv])
    return d


BRUSHED = dict(GOLD, alpha=0.05, alpha_v=0.3, twosided=True)


def test_anisotropic_conductor_renders_agree():
    """(a) the estimators agree on the mean: luminaire sampling on and off, guided and unguided; (b) swapping alphaU and alphaV and turning the
    texture coordinates by 90 degrees is the same surface: the tangent frame follows the UV tangents as Mitsuba's does"""
    from test_delta_emitters_gpu import _arm, _compare
    desc = _plate_scene(BRUSHED)
    a = _arm(desc, hideEmitters=0)
    assert a.mean() > 0 and np.isfinite(a).all()
    _compare("nee always vs never", a, _arm(desc, hideEmitters=0, nee="never"))
    _compare("guided vs unguided", a, _arm(desc, hideEmitters=0, bsdfSamplingFraction=1.0, bsdfSamplingFractionLoss="none"))
    _compare("alphas swapped, texture coordinates turned", a, _arm(_plate_scene(dict(BRUSHED, alpha=0.3, alpha_v=0.05), turned=True), hideEmitters=0))


def test_rough_pane_mean_does_not_depend_on_the_sampler():
    """(c) sampleVisible changes the variance, not the mean"""
    from test_delta_emitters_gpu import _arm, _compare
    pane = dict(type="roughdielectric", alpha=0.2, eta=1.5, reflectance=(1, 1, 1), specular=(1, 1, 1))
    a = _arm(_plate_scene(dict(pane, sample_visible=False)), hideEmitters=0)
    b = _arm(_plate_scene(dict(pane, alpha_v=0.2)), hideEmitters=0)
    _compare("sampleVisible false vs true", a, b)


def test_two_shards_in_one_process_equal_the_unsharded_film():
    """two contexts with shards 0 and 1 of 2, their buffers summed as a reducer would, against one context"""
    import torch
    import ppg_host
    from ppg_host.distributed import _view
    dev = torch.device("cuda", 0)
    w, h = 64, 48
    scene = _plate_scene(BRUSHED)
    props = dict(budgetType="spp", budget=47, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=23, sppPerPass=1)
    ref_gpt = ppg_host.GuidedPathTracer(engine=hip(**props))
    ref_img = ref_gpt.render(scene)
    schedule = [it["passes"] for it in ref_gpt.iterations]

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
            e.set_do_nee(True)
            e.begin_iteration(final)
        for e in engines:
            e.render_passes_nostat(p)
        if final:
            bufs = [e.final_partials() for e in engines]
            total([_view(torch, b_[0], b_[1], "<f4", dev) for b_ in bufs])
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
                    total([_view(torch, b_[k][0], b_[k][1], "<i8", dev) for b_ in bufs])
        for e in engines:
            e.build_sdtree(); e.end_iteration()
    for e in engines:
        e.end_render()
        assert np.array_equal(e.read_film(), ref_img)
        _tree_equal(e.read_sdtree(), ref_gpt.engine.read_sdtree())
    assert ref_img.mean() > 0


def test_cpp_driver_equals_python_on_the_converted_scene(tmp_path):
    import subprocess
    import ppg_host
    from test_cpp_host import read_pfm
    exe = os.path.join(os.path.dirname(GOLDEN), "..", "practical-path-guiding_amd", "bin", "ppg_render")
    path = str(tmp_path / "plate.ppgs")
    ppg_host.save_scene(_plate_scene(dict(BRUSHED, distribution="phong")), path)
    props = dict(budgetType="spp", budget=28, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=4, **{k: v for k, v in IMPROVED.items() if k != "sppPerPass"})
    out = str(tmp_path / "out.pfm")
    args = [exe, "-q", "-o", out] + sum([["-D", "%s=%s" % kv] for kv in props.items()], [])
    r = subprocess.run(args + [path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    back = ppg_host.load_scene_file(path)
    assert back.materials[-1]["alpha_v"] == float(f32(0.3)) and back.materials[-1]["distribution"] == "phong"
    img = ppg_host.GuidedPathTracer(engine=hip(**props)).render(back)
    assert np.array_equal(read_pfm(out), img) and img.mean() > 0
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(_plate_scene(dict(GOLD, alpha=0.05, twosided=True)))
    assert not np.array_equal(img, plain)


# ------------------------------------------------------------------------------------------------ host paths
def test_render_is_deterministic_and_a_cleared_list_equals_a_fresh_context():
    import ppg_host
    props = dict(CBOX_PROPS, budget=12, seed=3)
    plain = ppg_host.cbox_scene(16, 12)
    aniso = _box_scene(True)

    def render(e, desc):
        e.set_scene(desc)
        e.render()
        return e.read_film()
    e = hip(**props)
    a = render(e, aniso)
    b = render(e, plain)       # set_scene sends the empty list: the context's entries are cleared
    a2 = render(e, aniso)
    e.close()
    fresh = hip(**props)
    c = render(fresh, plain)
    fresh.close()
    assert np.array_equal(a, a2) and np.array_equal(b, c) and not np.array_equal(a, b)


def test_bad_lists_are_refused():
    import ppg_host
    from ppg_host.bindings import Microfacet, PPGError
    desc, base = scene_with([dict(GOLD), dict(type="roughplastic", alpha=0.2, eta=1.5, slice=rtrans_slice("beckmann", 0.2, 1.49)), dict(type="plastic")])
    n = len(desc.materials)
    e = hip(**dict(CBOX_PROPS, budget=4))

    def entries(k, **kw):
        out = [Microfacet() for _ in range(n)]
        out[k].general = 1
        out[k].alpha_v = kw.pop("alpha_v", desc.materials[k].get("alpha", 0.1))
        for name, v in kw.items():
            if name == "_reserved":
                out[k]._reserved[1] = v
            else:
                setattr(out[k], name, v)
        return out

    def refused(lst, needle):
        with pytest.raises(PPGError) as ei:
            _again(e, desc, lst)
        assert needle in str(ei.value), str(ei.value)
    refused(entries(base + 2), "only roughconductor")                       # general on a plastic
    refused(entries(base + 1, alpha_v=0.3), "anisotropic")                  # roughplastic with alphaV != alpha
    refused(entries(base + 1, alpha_v_texture=1), "alpha_v_texture")        # ... or with a bitmap
    refused(entries(base, _reserved=7), "_reserved")
    refused(entries(base, alpha_v_texture=5), "out of range")
    refused(entries(base, distribution=2), "distribution")
    refused(entries(base)[:-1], "entries")
    # an anisotropic material on a mesh without texture coordinates
    tm = np.array(desc.tri_material); tm[4] = base; desc.tri_material = tm
    refused(entries(base, alpha_v=0.4), "texture coordinates")
    e.close()


def _again(e, desc, lst):
    """set_scene with the list `lst` instead of the one the material dicts state"""
    import ppg_host.bindings as b
    orig = b.has_general_microfacet
    send = e.set_microfacet
    try:
        b.has_general_microfacet = lambda d: True
        e.set_microfacet = lambda entries: send(lst)
        e.set_scene(desc)
    finally:
        b.has_general_microfacet = orig
        del e.set_microfacet


def test_the_call_is_refused_inside_a_render():
    from ppg_host.bindings import PPGError
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(_box_scene(True))
    e.begin_render()
    with pytest.raises(PPGError) as ei:
        e.set_microfacet([])
    assert "ppg_begin_render" in str(ei.value)
    e.close()
