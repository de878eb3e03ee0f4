"""The coating / roughcoating adapters on the GPU (include/ppg.h ppg_set_coatings; csrc: the coat kernels, PPG_COAT):

  * the test hook ppg_debug_bsdf — the render's own mat_eval / mat_pdf / mat_sample — against the float64 restatement of test_coatings.py,
    for every allowed pairing, with and without the two-sided adapter, each case held to 8 x its own float32-against-float64 figure;
  * the coat family changes nothing else: a scene that merely holds a coated material, today's materials through it, an empty list;
  * renders of a coated box: estimators agree, bookkeeping is intact, and the coats show;
  * the C-ABI's refusals.
"""
import os

import numpy as np
import pytest

from conftest import CBOX_PROPS, IMPROVED
from test_bsdfs import GOLD, SMOOTH
from test_coatings import (CASES, DIFFUSE, MARGIN, NESTED, ROUGH_COATS, SMOOTH_COAT, case_id, coat_of, deviations, float32_figures, lattice,
                           reference)
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def with_slices(desc, materials):
    """`materials` appended to desc's own; the slices of roughplastics and roughcoatings (arrays under `slice`) gathered into desc.rtrans and
    replaced by their row"""
    rows = [] if getattr(desc, "rtrans", None) is None else [np.asarray(r, f32) for r in desc.rtrans]

    def row(sl):
        sl = np.asarray(sl, f32)
        for k, r in enumerate(rows):
            if np.array_equal(r, sl):
                return k
        rows.append(sl)
        return len(rows) - 1
    out = []
    for m in materials:
        m = dict(m)
        if "slice" in m:
            m["rtrans"] = row(m.pop("slice"))
        if m.get("coating") is not None and "slice" in m["coating"]:
            c = dict(m["coating"])
            c["rtrans"] = row(c.pop("slice"))
            m["coating"] = c
        out.append(m)
    base = len(desc.materials)
    desc.materials = list(desc.materials) + out
    desc.rtrans = np.stack(rows) if rows else None
    return base


def case_material(case):
    cname, nname, twosided = case
    m = dict(NESTED[nname], coating=dict(coat_of(cname)))
    if twosided:
        m["twosided"] = True
    return m


# ------------------------------------------------------------------------------------------------ 1. the hook against the restatement
@pytest.fixture(scope="module")
def hook():
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    base = with_slices(desc, [case_material(c) for c in CASES])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    out = {}
    for k, c in enumerate(CASES):
        wi, wo, u = lattice(c[2])
        out[c] = e.debug_bsdf(base + k, wi, wo, u)
    e.close()
    return out


class _S:
    def __init__(self, g):
        self.wo, self.pdf, self.weight, self.delta = g["wo"], g["sampled_pdf"], g["weight"], g["delta"] != 0


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_hook_equals_the_restatement(hook, case):
    """Bounds: 8 x what the restatement itself loses between float32 and float64 on these very items (test_coatings.py, measured there
    per case), never below 8 x 2^-23 — the margin of the general-microfacet tests, for their reason: the kernels' operation order differs
    from numpy's, their exp / pow / sincos are the library's own, and grazing directions cancel.
    Measured on an MI355X, largest over the cases — see DESIGN.md "Coatings"."""
    g = hook[case]
    ref = reference(case)
    fig, excluded, _ = float32_figures(case)
    dev = deviations(dict(eval=g["eval"], pdf=g["pdf"], sample=_S(g)), ref)
    floor = 2.0 ** -23
    print(case_id(case), "hook vs float64:", dev, "| float32 vs float64:", fig, "| excluded", excluded)
    keep, s = ref["keep"], ref["sample"]
    assert np.isfinite(g["eval"]).all() and np.isfinite(g["pdf"]).all() and np.isfinite(g["weight"]).all() and np.isfinite(g["wo"]).all()
    # flags, on every item outside the exclusion rule (an item within MARGIN of a branch point, test_coatings.py)
    assert MARGIN == 1e-4
    ok = g["weight"].any(1)
    assert np.array_equal(ok[keep], s.weight.any(1)[keep])
    assert np.array_equal((g["delta"] != 0)[keep & ok], s.delta[keep & ok])
    assert not g["is_null"].any()
    assert np.all(g["eta"][keep & ok] == 1)
    for name in ("eval", "pdf", "weight", "sampled_pdf", "direction"):
        assert dev[name] <= 8 * max(fig[name], floor), (name, dev[name], fig[name])


# ------------------------------------------------------------------------------------------------ 2. the family changes nothing else
def _render(desc, **props):
    e = hip(**dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=11, nee="always", **props))
    e.set_scene(desc)
    e.render()
    out = e.read_film(), e.read_sdtree()
    e.close()
    return out


UNUSED_COATED = dict(DIFFUSE, coating=dict(SMOOTH_COAT))


def test_a_scene_that_only_holds_a_coated_material_renders_the_same_bits():
    import ppg_host
    path = os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs")
    fa, ta = _render(ppg_host.load_scene_file(path))
    desc = ppg_host.load_scene_file(path)
    with_slices(desc, [UNUSED_COATED])  # on no triangle: the coat kernels run, and meet no coat
    fb, tb = _render(desc)
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


def _smooth_box(coated):
    """the box's 24 triangles on test_bsdfs.SMOOTH's materials; an unused general microfacet entry sends it through the extended kernels,
    an unused coat on top of that through the coat kernels"""
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    mats = [dict(m) for _, m in SMOOTH]
    base = with_slices(desc, mats + [dict(GOLD, alpha_v=0.1), UNUSED_COATED if coated else DIFFUSE])
    tm = np.array(desc.tri_material)
    box = np.nonzero(tm == 0)[0]
    assert len(box) == 24
    tm[box] = base + np.arange(24) * len(mats) // 24
    desc.tri_material = tm
    return desc


def test_todays_materials_through_the_coat_kernels_equal_the_extended_kernels():
    fa, ta = _render(_smooth_box(False))
    fb, tb = _render(_smooth_box(True))
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


def test_a_list_without_a_coat_equals_no_list():
    import ppg_host
    fa, ta = _render(ppg_host.cbox_scene(16, 12))
    desc = ppg_host.cbox_scene(16, 12)
    desc.materials = [dict(m, coating=dict(kind=0)) for m in desc.materials]
    fb, tb = _render(desc)
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


# ------------------------------------------------------------------------------------------------ 3., 4. renders of a coated box
W, H = 64, 48
FLOOR_COAT = dict(kind="coating", eta=1.5, thickness=1.0, sigma_a=(0.8, 0.3, 0.1))
WALL_COAT = dict(ROUGH_COATS["ggx"])
SPP = 4095  # (4092 where a pass has 4): iterations of 1, 2, 4, .. passes and a last one of 2048 spp; one standard error of the mean image radiance is then
#             below 1 % of the mean in all four renders (asserted; measured 0.2 % .. 0.5 %)
LAST_SPP = 2048


def coated_box(coats=True):
    """the Cornell box with the floor a tinted coating over its diffuse white and the back wall a roughcoating over GOLD (coats = False:
    the same two materials bare)"""
    import ppg_host
    desc = ppg_host.cbox_scene(W, H)
    pos, idx = np.asarray(desc.positions), np.asarray(desc.indices)
    tri = pos[idx]  # [n, 3, 3]
    floor = np.all(tri[:, :, 1] == 0, axis=1) & (np.asarray(desc.tri_material) == 1)  # (the boxes stand on it: "white" alone)
    back = np.all(np.abs(tri[:, :, 2] - 559.20001) < 1e-3, axis=1)
    assert floor.sum() == 2 and back.sum() == 2
    white = dict(desc.materials[np.asarray(desc.tri_material)[floor][0]])
    a, b = dict(white), dict(GOLD)
    if coats:
        a["coating"], b["coating"] = dict(FLOOR_COAT), dict(WALL_COAT)
    base = with_slices(desc, [a, b])
    tm = np.array(desc.tri_material)
    tm[floor], tm[back] = base, base + 1
    desc.tri_material = tm
    return desc


def _last_iteration_spp(budget, spp_per_pass):
    """the schedule of renderSPP: iterations of 1, 2, 4, .. passes, the last one taking what is left when less than two more would fit"""
    n = -(-budget // spp_per_pass)
    done, it = 0, 0
    while True:
        rem = n - done
        this = min(rem, 1 << it)
        if rem - this < 2 * this:
            return rem * spp_per_pass
        done += this
        it += 1


_renders = {}


def box_render(which):
    """film, per-pixel standard error of the last iteration (ppg_read_variance: the variance of that iteration's samples), stats"""
    if which not in _renders:
        common = dict(budgetType="spp", maxDepth=-1, rrDepth=5, seed=3)
        props = {
            "nee-always": dict(common, budget=SPP - 3, sppPerPass=4, nee="always", sampleCombination="discard"),
            "nee-never": dict(common, budget=SPP - 3, sppPerPass=4, nee="never", sampleCombination="discard"),
            "guided": dict(IMPROVED, **common, budget=SPP, nee="never"),
            "unguided": dict(IMPROVED, **common, budget=SPP, nee="never", bsdfSamplingFraction=1.0, bsdfSamplingFractionLoss="none"),
            "bare": dict(common, budget=SPP - 3, sppPerPass=4, nee="always", sampleCombination="discard"),
        }[which]
        assert _last_iteration_spp(props["budget"], props["sppPerPass"]) == LAST_SPP
        e = hip(**props)
        e.set_scene(coated_box(which != "bare"))
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
def test_estimators_agree_on_a_coated_box(pair):
    (ma, sa), (mb, sb) = _mean_and_se(pair[0]), _mean_and_se(pair[1])
    print(pair, "mean", ma, mb, "standard error", sa, sb, "relative", sa / ma, sb / mb, "spp", SPP)
    assert np.all(sa < 0.01 * ma) and np.all(sb < 0.01 * mb)
    assert np.all(np.abs(ma - mb) <= 4 * np.sqrt(sa * sa + sb * sb)), (ma - mb) / np.sqrt(sa * sa + sb * sb)


def test_bookkeeping_of_a_coated_box():
    """the invariants of test_gpu_parity.test_full_size_invariants on this scene: samples and rays add up, and with the nearest filters
    every committed vertex carries weight 1 into exactly one leaf"""
    for nee in ("always", "never"):
        e = hip(budgetType="spp", budget=60, maxDepth=-1, rrDepth=5, seed=5, nee=nee)
        e.set_scene(coated_box()); e.begin_render()
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


def test_the_coats_show():
    """without the coats the floor is another picture: the test that fails when a host drops the entries"""
    rows = slice(H - 6, H)  # the bottom rows see the floor
    (ma, sa), (mb, sb) = _mean_and_se("nee-always", rows), _mean_and_se("bare", rows)
    print("floor rows: coated", ma, "bare", mb, "standard errors", sa, sb)
    assert np.all(np.abs(ma - mb) > 4 * np.sqrt(sa * sa + sb * sb))


# ------------------------------------------------------------------------------------------------ 5. the refusals
def _coating(**kw):
    from ppg_host.bindings import Coating
    c = Coating.from_dict(dict(dict(kind=2, eta=1.5, alpha=0.1, distribution="ggx", rtrans=0), **kw))
    return c


def _reserved():
    c = _coating(kind=0)
    c._reserved[1] = 7
    return c


REFUSALS = [  # (name, nested material, the entry, what the message says)
    ("dielectric", dict(type="dielectric", eta=1.5), lambda: _coating(kind=1), "dielectric"),
    ("thindielectric", dict(type="thindielectric", eta=1.5), lambda: _coating(kind=1), "dielectric"),
    ("roughdielectric", dict(type="roughdielectric", eta=1.5, alpha=0.2), lambda: _coating(), "dielectric"),
    ("roughcoating-conductor", dict(type="conductor", eta=GOLD["eta"], k=GOLD["k"]), lambda: _coating(), "delta"),
    ("roughcoating-mirror", dict(type="mirror"), lambda: _coating(), "delta"),
    ("roughcoating-plastic", dict(type="plastic", eta=1.49), lambda: _coating(), "delta"),
    ("kind", DIFFUSE, lambda: _coating(kind=3), "kind"),
    ("eta-zero", DIFFUSE, lambda: _coating(eta=0.0), "indices of refraction"),
    ("eta-negative", DIFFUSE, lambda: _coating(eta=-1.5), "indices of refraction"),
    ("eta-one", DIFFUSE, lambda: _coating(eta=1.0), "indices of refraction"),
    ("eta-nan", DIFFUSE, lambda: _coating(eta=float("nan")), "finite"),
    ("thickness-inf", DIFFUSE, lambda: _coating(thickness=float("inf")), "finite"),
    ("sigma-nan", DIFFUSE, lambda: _coating(sigma_a=(0, float("nan"), 0)), "finite"),
    ("specular-inf", DIFFUSE, lambda: _coating(specular=(1, 1, float("inf"))), "finite"),
    ("alpha-nan", DIFFUSE, lambda: _coating(alpha=float("nan")), "finite"),
    ("thickness-negative", DIFFUSE, lambda: _coating(thickness=-1.0), "thickness"),
    ("sigma-negative", DIFFUSE, lambda: _coating(sigma_a=(0.1, -0.1, 0)), "sigma_a"),
    ("distribution", DIFFUSE, lambda: _coating(distribution=3), "distribution"),
    ("slice-high", DIFFUSE, lambda: _coating(rtrans=1), "rtrans"),
    ("slice-negative", DIFFUSE, lambda: _coating(rtrans=-1), "rtrans"),
    ("reserved", DIFFUSE, _reserved, "_reserved"),
]


@pytest.fixture(scope="module")
def engine():
    e = hip(**dict(CBOX_PROPS, budget=4))
    yield e
    e.close()


def _scene(nested):
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    desc.materials = list(desc.materials) + [dict(nested)]
    desc.rtrans = np.asarray(ROUGH_COATS["ggx"]["slice"], f32)[None]
    return desc


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_material_and_leave_the_context_usable(engine, k):
    import ppg_host
    from ppg_host.bindings import Coating, PPGError
    name, nested, entry, says = REFUSALS[k]
    desc = _scene(nested)
    n = len(desc.materials)
    desc.coatings = [Coating() for _ in range(n - 1)] + [entry()]
    with pytest.raises(PPGError) as err:
        engine.set_scene(desc)
    assert err.value.code == -1  # PPG_ERR_INVALID
    assert "material %d" % (n - 1) in str(err.value) and says in str(err.value), str(err.value)
    # the list is kept until it is replaced: the same scene is refused again, and accepted once the entry is in order
    good = _scene(DIFFUSE)
    good.coatings = [Coating() for _ in range(n - 1)] + [_coating()]
    engine.set_scene(good)
    out = engine.debug_bsdf(n - 1, [0, 0, 1], np.array([[0.3, 0.2, 0.9]], f32), [0.5, 0.5])
    assert out["eval"].any() and np.isfinite(out["eval"]).all()


def test_list_length_and_state(engine):
    import ppg_host
    from ppg_host.bindings import Coating, PPGError
    desc = _scene(DIFFUSE)
    n = len(desc.materials)
    for length in (1, n - 1, n + 1):
        desc.coatings = [Coating() for _ in range(length)]
        with pytest.raises(PPGError) as err:
            engine.set_scene(desc)
        assert err.value.code == -1 and "%d entries" % length in str(err.value) and "%d materials" % n in str(err.value)
    desc.coatings = []  # n_materials = 0 clears the list
    engine.set_scene(desc)
    engine.begin_render()
    with pytest.raises(PPGError) as err:
        engine.set_coatings([Coating() for _ in range(n)])
    assert err.value.code == -3  # PPG_ERR_STATE
    engine.end_render()
    desc.coatings = [Coating() for _ in range(n - 1)] + [_coating(kind=1)]
    engine.set_scene(desc)
    engine.render()
    assert np.isfinite(engine.read_film()).all()
