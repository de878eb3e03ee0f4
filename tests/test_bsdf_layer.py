"""The BSDF layer of the oracle against a float64 restatement written in this repository (bsdf_ref.py), item by item over the cases of
bsdf_cases.py, and its known answers at the edges; the hook ppg_debug_bsdf_as holds every compiled copy of the kernels' layer to the oracle
bit for bit (test_bsdf_layer_gpu.py).

The comparison's bar per value is (4 s + k) ulp of the value: s is the spread of the float64 result when every float32 input moves by one
ulp (the problem's own conditioning), k the material's figure of K_ULPS — twice the largest distance that remained
between oracle and restatement over the unflagged items when the table was measured, rounded up (`python tests/test_bsdf_layer.py` prints
the measurement).  An item is boundary-flagged, and left out of THIS comparison only, when the restatement's branch signature changes
under such a move.  A direction component moves to its float32 neighbours; a sample coordinate moves by max(its ulp, 2^-24): the plug-ins
first form 2 u - 1 or u / p, whose rounding is of that absolute size wherever u sits in [0, 1).  The spread also takes in one float32 ulp of
the dielectric Fresnel reflectance, the one intermediate the plug-ins round and then subtract from 1 (bsdf_ref.F_ULPS): at |wi.z| <= 2^-12
the differences 1 - F and 1 - R^2 keep no digit in float32 whatever the inputs, and the distance there was 4e5 .. 1e7 ulp without it."""
import ctypes as C

import numpy as np
import pytest

import bsdf_cases as bc
import bsdf_ref as br
from ppg_host.bindings import Material
from test_bsdfs import _fp, _slice, bsdf_eval

f32, f64 = np.float32, np.float64
IP = C.POINTER(C.c_int32)


# ------------------------------------------------------------------------------------------------ the oracle's entries
def oracle_sample(lib, mat, wi, u):
    """ppgo_bsdf_sample_ex: item i draws roughdielectric's extra number from path_key(77, i, 0)"""
    _slice(lib, mat)
    m = Material.from_dict(mat)
    n = len(u)
    wi, u = np.ascontiguousarray(wi, f32), np.ascontiguousarray(u, f32)
    out = dict(wo=np.zeros((n, 3), f32), weight=np.zeros((n, 3), f32), pdf=np.zeros(n, f32), eta=np.zeros(n, f32), delta=np.zeros(n, np.int32),
               null=np.zeros(n, np.int32))
    assert lib.ppgo_bsdf_sample_ex(C.byref(m), n, _fp(wi), _fp(u), _fp(out["wo"]), _fp(out["weight"]), _fp(out["pdf"]), _fp(out["eta"]),
                                   out["delta"].ctypes.data_as(IP), out["null"].ctypes.data_as(IP)) == 0
    return out


def oracle_flags(lib, mat):
    """-> the bits of ppg_debug_bsdf_out._pad[0]: smooth, backside or transmission, has a null component"""
    _slice(lib, mat)
    m = Material.from_dict(mat)
    a, b, c, d = (C.c_int32() for _ in range(4))
    assert lib.ppgo_bsdf_flags(C.byref(m), C.byref(a), C.byref(b), C.byref(c)) == 0
    assert lib.ppgo_bsdf_has_null(C.byref(m), C.byref(d)) == 0
    assert a.value in (0, 1) and b.value == 1 - a.value
    return (1 if a.value else 0) | (2 if c.value else 0) | (4 if d.value else 0)


_oracle_cache = {}


def oracle_all(lib, name):
    """eval, pdf and the sample record of every item of material `name`, computed once"""
    if name not in _oracle_cache:
        mat, it = dict(bc.MATERIALS)[name], bc.items(name)
        f, p = bsdf_eval(lib, mat, it["wi"], it["wo"])
        _oracle_cache[name] = dict(oracle_sample(lib, mat, it["wi"], it["u"]), eval=f, epdf=p, flags=oracle_flags(lib, mat))
        for v in _oracle_cache[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _oracle_cache[name]


# ------------------------------------------------------------------------------------------------ conditioning and branch flags
def _moves(x, sample):
    """the 2 d neighbours of float32 [n, d]: one coordinate at a time, down and up"""
    for c in range(x.shape[1]):
        for up in (False, True):
            y = x.copy()
            if sample:
                step = np.maximum(np.spacing(x[:, c]), f32(2.0 ** -24))
                y[:, c] = np.clip(x[:, c] + (step if up else -step), f32(0), np.nextafter(f32(1), f32(0)))
            else:
                y[:, c] = np.clip(np.nextafter(x[:, c], f32(np.inf if up else -np.inf)), f32(-1), f32(1))  # (a direction's component stays one)
            yield y


def conditioned(fn, a, b, b_is_sample):
    """fn(a, b) -> (dict of float64 arrays, signature).  -> (values, spread per value, flagged): the spread is max - min over the item and
    its neighbours, an item is flagged when a neighbour's signature differs (or a value is not finite)"""
    base, sig = fn(a, b)
    lo, hi = {k: v.copy() for k, v in base.items()}, {k: v.copy() for k, v in base.items()}
    flagged = np.zeros(len(a), bool)
    for k, v in base.items():
        flagged |= ~np.isfinite(v.reshape(len(a), -1)).all(1)
    for which in (0, 1):
        for y in _moves((a, b)[which], which == 1 and b_is_sample):
            r, s = fn(*((y, b) if which == 0 else (a, y)))
            flagged |= s != sig
            for k in base:
                with np.errstate(invalid="ignore"):
                    lo[k], hi[k] = np.minimum(lo[k], r[k]), np.maximum(hi[k], r[k])
                    flagged |= ~np.isfinite(r[k].reshape(len(a), -1)).all(1)
    for shift in (-1, 1):  # ... and the one rounded intermediate the plug-ins subtract from 1 (bsdf_ref.F_ULPS)
        br.F_ULPS = shift
        try:
            r, s = fn(a, b)
        finally:
            br.F_ULPS = 0
        flagged |= s != sig
        for k in base:
            with np.errstate(invalid="ignore"):
                lo[k], hi[k] = np.minimum(lo[k], r[k]), np.maximum(hi[k], r[k])
    return base, {k: hi[k] - lo[k] for k in base}, flagged


def ulp32(v):
    return np.spacing(np.abs(v).astype(f32)).astype(f64)


def remaining_ulps(got, ref, spread):
    """what is left of |got - ref| beyond 4 s, in ulps of the value"""
    with np.errstate(invalid="ignore"):
        return np.maximum(0.0, np.abs(got.astype(f64) - ref) - 4 * spread) / ulp32(ref)


def compare(lib, name):
    """-> dict(eval_flagged, sample_flagged, sample_known [n], rest = {quantity: remaining ulps [n] or [n, 3]}, exact = {quantity: equal [n]})"""
    mat, it, o = dict(bc.MATERIALS)[name], bc.items(name), oracle_all(lib, name)
    P = br.Params(mat)

    def ev(wi, wo):
        f, p, s = br.eval_pdf(P, wi, wo)
        return dict(eval=f, epdf=p), s

    def sm(wi, u):
        r = br.sample(P, wi, u)
        live = r["weight"].any(1)  # (a failed sample leaves the rest of the record unspecified)
        sig = r["sig"] | (r["delta"].astype(np.int64) << 40) | (r["null"].astype(np.int64) << 41) | (r["known"].astype(np.int64) << 42)
        return dict(weight=r["weight"], wo=np.where(live[:, None], r["wo"], 0.0), pdf=np.where(live, r["pdf"], 0.0), eta=np.where(live, r["eta"], 1.0)), sig

    eb, es, ef = conditioned(ev, it["wi"], it["wo"], False)
    sb, ss, sf = conditioned(sm, it["wi"], it["u"], True)
    # A direction built within four ulps of the critical angle, and a sample within three ulps of a lobe threshold (EDGE builds the rounded
    # threshold's neighbours up to two ulps away), sit on a branch by construction: the quantity the branch compares with is itself a rounded
    # float32 expression (the square root at the critical angle, a ratio of 1 - F terms), not an input.
    built_on = (it["wi_class"] == "critical")
    near = np.zeros(len(built_on), bool)
    for axis, t in br.thresholds(P, it["wi"]):
        with np.errstate(invalid="ignore"):
            near |= np.abs(it["u"][:, axis].astype(f64) - t) <= 3 * ulp32(t)
    ef, sf = ef | built_on, sf | built_on | near
    r = br.sample(P, it["wi"], it["u"])
    live = r["weight"].any(1) & o["weight"].any(1)  # (a failed sample leaves the rest of the record unspecified; `weight` itself is compared everywhere)
    rest = {k: remaining_ulps(o[k], eb[k], es[k]) for k in ("eval", "epdf")}
    rest["weight"] = remaining_ulps(o["weight"], sb["weight"], ss["weight"])
    for k in ("wo", "pdf", "eta"):
        w = live if o[k].ndim == 1 else live[:, None]
        rest[k] = np.where(w, remaining_ulps(o[k], sb[k], ss[k]), 0.0)
    exact = dict(delta=~live | (o["delta"] == r["delta"]), null=~live | (o["null"] == r["null"]))
    return dict(eval_flagged=ef, sample_flagged=sf, sample_known=r["known"], rest=rest, exact=exact)


# Measured on the CPU by `python tests/test_bsdf_layer.py` (measure() below): the largest distance that remains over the unflagged items,
# per material and item set, doubled and rounded up.  The restatement states D, G1 and the Fresnel terms from the formulas, the oracle
# follows the plug-ins' float32 expression order: what remains after the conditioning is the rounding of that order.  plastic's figure is
# the internal diffuse Fresnel reflectance, an integral each side computes by its own quadrature: the reference integrates it to 1e-5
# (util.cpp:797-861), the oracle's Simpson rule (include/ppg_detmath.h) and the restatement's differ by 9.4e-6 and 2.9e-6 in it for the
# two indices used here, 2.3e-5 and 2.5e-6 of the diffuse term.  DESIGN.md section 5 repeats the table with the flagged shares.
K_ULPS = {  # name: (LATTICE, EDGE)
    'diffuse': (1, 0),
    'twosided-diffuse': (1, 0),
    'ggx-0.25': (21, 12),
    'ggx-0.05': (24, 20),
    'ggx-0.6-twosided': (21, 18),
    'ggx-beckmann-0.25': (4, 0),
    'ggx-beckmann-0.08': (0, 0),
    'ggx-beckmann-0.5': (9, 5),
    'ggx-roughdielectric-0.3': (16, 9),
    'ggx-roughdielectric-beckmann-0.15': (0, 0),
    'ggx-roughplastic-0.1': (9, 5),
    'ggx-roughplastic-beckmann-0.2-nonlinear-twosided': (8, 5),
    'plastic': (771, 768),
    'plastic-nonlinear': (98, 68),
    'mirror': (0, 0),
    'conductor-gold': (16, 16),
    'conductor-k0': (8, 16),
    'dielectric-1.5': (3, 3),
    'dielectric-inv1.5': (2, 2),
    'dielectric-1': (0, 0),
    'thindielectric-1.5': (0, 0),
    'plastic-twosided': (771, 768),
    'roughplastic-coloured-specular': (8, 3),
    'roughdielectric-inv1.5': (18, 6),
    'roughconductor-alpha-floor': (23, 15),
    'roughconductor-alpha-1': (27, 21),
    'mask-diffuse': (4, 3),
    'mask-0-diffuse': (0, 0),
    'mask-1-diffuse': (1, 0),
    'mask-twosided-roughconductor': (25, 23),
    'mask-dielectric': (5, 5),
}


def worst_remaining(c, it, edge):
    """the largest remaining distance of one comparison over the unflagged items of LATTICE (edge = False) or EDGE"""
    sel = it["is_edge"] == edge
    ok_e, ok_s = ~c["eval_flagged"] & sel, ~c["sample_flagged"] & c["sample_known"] & sel
    out = {q: float(c["rest"][q][ok_e].max()) if ok_e.any() else 0.0 for q in ("eval", "epdf")}
    out.update({q: float(c["rest"][q][ok_s].max()) if ok_s.any() else 0.0 for q in ("weight", "wo", "pdf", "eta")})
    return out, ok_e, ok_s


@pytest.fixture(scope="module")
def compared(oracle_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = compare(oracle_lib, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", bc.NAMES)
def test_lattice_stays_clear_of_the_branches(compared, name):
    """at most 1 % of a material's LATTICE is boundary-flagged: the lattice was built to stay clear of the branches"""
    c, lat = compared(name), ~bc.items(name)["is_edge"]
    print(name, "flagged share of LATTICE: eval", c["eval_flagged"][lat].mean(), "sample", c["sample_flagged"][lat].mean())
    assert c["eval_flagged"][lat].mean() <= 0.01 and c["sample_flagged"][lat].mean() <= 0.01


@pytest.mark.parametrize("edge", [False, True], ids=["LATTICE", "EDGE"])
@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_equals_the_float64_restatement(compared, name, edge):
    c, it = compared(name), bc.items(name)
    worst, ok_e, ok_s = worst_remaining(c, it, edge)
    print(name, "EDGE" if edge else "LATTICE", "compared", int(ok_e.sum()), "eval items,", int(ok_s.sum()), "sample items; remaining ulps", worst)
    assert ok_e.sum() >= (0.99 if not edge else 0.4) * (it["is_edge"] == edge).sum()
    for q, v in worst.items():
        assert v <= K_ULPS[name][int(edge)], q
    for q in ("delta", "null"):
        assert c["exact"][q][ok_s].all(), q


def test_every_sample_routine_the_restatement_covers_is_compared(compared):
    """the sampling half compares at least a fifth of the LATTICE of every material whose sample() the restatement states (all but the
    bare roughconductor and roughdielectric, whose every sample needs the microfacet normal)"""
    for name, mat in bc.MATERIALS:
        c, lat = compared(name), ~bc.items(name)["is_edge"]
        covered = (~c["sample_flagged"] & c["sample_known"])[lat].mean()
        if mat["type"] in ("roughconductor", "roughdielectric") and mat.get("opacity") is None:
            assert covered == 0
        else:
            assert covered > 0.2, name


# ------------------------------------------------------------------------------------------------ known answers at the edges, exact
def _mat(name):
    return dict(bc.MATERIALS)[name]


def _one_sided_brdf(mat):
    return mat["type"] in ("diffuse", "plastic", "roughconductor", "roughplastic", "mirror", "conductor") and not mat.get("twosided")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("name", [n for n, m in bc.MATERIALS if _one_sided_brdf(m)])
def test_one_sided_brdfs_are_black_from_the_horizon_down(oracle_lib, name):
    """eval and pdf test wi.z <= 0 (diffuse.cpp:112-114, roughconductor.cpp:258-262, plastic.cpp:253-256, roughplastic.cpp:331-335), +0 and
    -0 included; so does every sample() but roughconductor's (below)"""
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    below = it["wi"][:, 2] <= 0
    assert below.sum() > 300 and np.isin(["horizon+0", "horizon-0"], it["wi_class"][below]).all()
    assert not bits(o["eval"][below]).any() and not bits(o["epdf"][below]).any()
    assert not o["weight"][below & (o["null"] == 0)].any()  # (a mask's pass-through is no sample of the BRDF)


@pytest.mark.parametrize("name", ["ggx-0.25", "ggx-beckmann-0.25", "roughconductor-alpha-floor", "roughconductor-alpha-1"])
def test_roughconductor_sample_on_the_horizon(oracle_lib, name):
    """Pinned.  roughconductor.cpp:370 refuses wi.z < 0, not wi.z <= 0, so wi.z == 0 reaches the sampler; with the visible normals the
    density of the sampled normal is then 0 (microfacet.h:349-351: pdfVisible returns 0 for cosTheta(wi) == 0) and sample() returns black
    at roughconductor.cpp:385-386.  The oracle knows no other sampler, so on it the two comparisons are indistinguishable; the kernels'
    copy with all normals sampled is held to the `<` in test_bsdf_layer_gpu.py."""
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    hor = it["wi"][:, 2] == 0
    assert hor.sum() == 288 and np.signbit(it["wi"][hor, 2]).sum() == 144
    assert not o["weight"][hor].any() and not bits(o["pdf"][hor]).any() and not bits(o["wo"][hor]).any()


@pytest.mark.parametrize("name", ["ggx-roughdielectric-0.3", "ggx-roughdielectric-beckmann-0.15", "roughdielectric-inv1.5"])
def test_roughdielectric_eval_is_black_on_the_horizon(oracle_lib, name):
    """roughdielectric.cpp:271: eval() returns 0 for cosTheta(wi) == 0, for every wo"""
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    hor = it["wi"][:, 2] == 0
    assert hor.sum() == 288 and not bits(o["eval"][hor]).any()


@pytest.mark.parametrize("name", ["twosided-diffuse", "plastic-twosided"])
def test_two_sided_flip_at_minus_zero(oracle_lib, name):
    """Pinned.  twosided.cpp:163: sample() flips for cosTheta(wi) < 0, which -0 is not: the nested BRDF sees wi.z = -0 <= 0 and fails.
    The oracle's eval() / pdf() flip unless wi.z > 0 (the nested BRDF from the other side, twosided.cpp:126-137 read for a surface that has
    one BRDF on both sides): -0 becomes +0, and the nested BRDF is black there all the same.  Either way nothing comes back at wi.z = -0,
    and at the smallest wi.z below it both flips act: the record is the mirror image of the one at +|wi.z|."""
    mat = _mat(name)
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    mz = (it["wi"][:, 2] == 0) & np.signbit(it["wi"][:, 2])
    assert mz.sum() == 144
    assert not o["weight"][mz].any() and not bits(o["eval"][mz]).any() and not bits(o["epdf"][mz]).any()
    g = (it["wi_class"] == "grazing") & (it["wi"][:, 2] < 0)
    up = it["wi"][g] * np.array([1, 1, -1], f32)
    f, p = bsdf_eval(oracle_lib, mat, up, it["wo"][g] * np.array([1, 1, -1], f32))
    assert np.array_equal(bits(f), bits(o["eval"][g])) and np.array_equal(bits(p), bits(o["epdf"][g])) and f.any()
    s = oracle_sample(oracle_lib, mat, up, it["u"][g])
    live = s["weight"].any(1)
    assert live.sum() > 100 and np.array_equal(bits(s["weight"]), bits(o["weight"][g])) and np.array_equal(bits(s["pdf"]), bits(o["pdf"][g]))
    assert np.array_equal(bits(s["wo"][live] * np.array([1, 1, -1], f32)), bits(o["wo"][g][live]))


@pytest.mark.parametrize("name", ["dielectric-1.5", "dielectric-inv1.5", "mask-dielectric"])
def test_total_internal_reflection(oracle_lib, name):
    """dielectric.cpp:284-296 with F = 1 (util.cpp:661-664): every sample reflects, pdf 1, weight = the specular reflectance (times the
    mask's opacity / its luminance where there is one: mask.cpp:190-197)"""
    mat = _mat(name)
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    P = br.Params(mat)
    prob = oracle_prob(oracle_lib, mat) if P.masked else f32(1)
    assert abs(float(prob) - float(br.lum(P.opacity) if P.masked else 1)) < 1e-6
    m = (it["wi_class"] == "inside-tir") & (it["u"][:, 0] < prob)
    assert m.sum() > 20
    want = np.array(mat["reflectance"], f32)
    if P.masked:
        want = want * np.array(mat["opacity"], f32) / oracle_prob(oracle_lib, mat)
    assert np.array_equal(bits(o["weight"][m]), np.broadcast_to(bits(want), (m.sum(), 3)))
    assert np.array_equal(o["pdf"][m], np.full(m.sum(), 1 if not P.masked else oracle_prob(oracle_lib, mat), f32))
    assert np.array_equal(bits(o["wo"][m]), bits(it["wi"][m] * np.array([-1, -1, 1], f32))) and o["delta"][m].all() and not o["null"][m].any()
    assert np.all(o["eta"][m] == 1)


def oracle_prob(lib, mat):
    """the mask's probability of the nested BSDF as the oracle forms it: the density of a pass-through is 1 - prob (mask.cpp:169-176)"""
    s = oracle_sample(lib, mat, np.array([[0, 0, 1]], f32), np.array([[np.nextafter(f32(1), f32(0)), 0.5]], f32))
    assert s["null"][0] == 1
    return f32(1) - s["pdf"][0]


def test_index_matched_dielectric(oracle_lib):
    """util.cpp:654-657: eta == 1 gives F = 0 and cosThetaT = -cosThetaI, so every sample with u.x > 0 goes straight on, wo = -wi exactly,
    weight = the specular transmittance, eta = 1; u.x = 0 takes `sample.x <= F` (dielectric.cpp:284) and reflects with density F = 0"""
    mat = _mat("dielectric-1")
    it, o = bc.items("dielectric-1"), oracle_all(oracle_lib, "dielectric-1")
    t = it["u"][:, 0] > 0
    assert np.array_equal(bits(o["wo"][t]), bits(-it["wi"][t])) and np.all(o["pdf"][t] == 1) and np.all(o["eta"][t] == 1)
    assert np.array_equal(bits(o["weight"][t]), np.broadcast_to(bits(np.array(mat["specular"], f32)), (t.sum(), 3)))
    r = ~t
    assert r.sum() > 100 and np.all(o["pdf"][r] == 0) and np.array_equal(bits(o["wo"][r]), bits(it["wi"][r] * np.array([-1, -1, 1], f32)))


def test_mask_pass_through(oracle_lib):
    """mask.cpp:169-176: opacity 0 always passes (wo = -wi, the null component, weight (1 - opacity) / (1 - prob) = 1), opacity 1 never does"""
    it, o = bc.items("mask-0-diffuse"), oracle_all(oracle_lib, "mask-0-diffuse")
    assert o["null"].all() and o["delta"].all() and np.all(o["weight"] == 1) and np.all(o["pdf"] == 1) and np.all(o["eta"] == 1)
    assert np.array_equal(bits(o["wo"]), bits(-it["wi"]))
    assert not bits(o["eval"]).any() and not bits(o["epdf"]).any()
    o1, od = oracle_all(oracle_lib, "mask-1-diffuse"), oracle_all(oracle_lib, "diffuse")
    assert not o1["null"].any() and not o1["delta"].any()
    for q in ("eval", "epdf", "weight", "wo", "pdf"):  # ... and is the nested BSDF itself
        assert np.array_equal(bits(o1[q]), bits(od[q])), q


@pytest.mark.parametrize("name", ["mirror", "conductor-gold", "conductor-k0", "dielectric-1.5", "dielectric-inv1.5", "dielectric-1", "thindielectric-1.5"])
def test_delta_plugins_are_black_in_solid_angle(oracle_lib, name):
    """conductor.cpp:222-230, dielectric.cpp:221-233, thindielectric.cpp:166-176: without EDiscrete in the measure eval() and pdf() are 0 for
    every wo — the exact mirror and refracted directions are among the items"""
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    assert np.isin(["reflect", "refracted", "minus-wi"], it["wo_class"]).all()
    assert not bits(o["eval"]).any() and not bits(o["epdf"]).any()


@pytest.mark.parametrize("name", ["diffuse", "mask-1-diffuse"])
def test_diffuse_sample_at_the_rim_of_the_disk(oracle_lib, name):
    """Pinned.  A sample the concentric map sends to the disk's rim gives z = 0, which warp.cpp:47-49 replaces by 1e-10f: diffuse.cpp:144-149
    then returns wo.z = 1e-10f, pdf = INV_PI * 1e-10f — tiny, not 0 — and weight = the reflectance.  (u = (0, 1/2) lands on (-1, 0) exactly.)"""
    mat = _mat(name)
    s = oracle_sample(oracle_lib, mat, np.array([[0, 0, 1], [0.6, 0, 0.8]], f32), np.array([[0, 0.5], [0, 0.5]], f32))
    assert np.all(s["wo"][:, 2] == f32(1e-10)) and np.all(s["wo"][:, 0] == -1)
    assert np.all(s["pdf"] == f32(f32(1 / np.pi) * f32(1e-10))) and np.all(s["pdf"] > 0)
    assert np.array_equal(bits(s["weight"]), np.broadcast_to(bits(np.array(mat["reflectance"], f32)), (2, 3)))
    it, o = bc.items(name), oracle_all(oracle_lib, name)
    rim = (o["wo"][:, 2] == f32(1e-10)) & o["weight"].any(1)
    assert rim.sum() >= 20  # (the EDGE grid's corners and edge midpoints)


def test_beckmann_density_underflows_to_zero(oracle_lib):
    """The finding of DESIGN.md section 5.  microfacet.h:203 evaluates exp(-tan^2 / alpha^2) / (pi alpha^2 cos^4) with math::fastexp, which
    underflows to 0 for a normal near the horizon; ppg_exp is clamped at exp(-80) = 1.8e-35, and divided by cos^4 of a normal 6e-8 above
    the horizon that came out as a density of 1e-5 and more.  wi = wo grazing makes such a half vector."""
    for name in ("ggx-beckmann-0.25", "ggx-beckmann-0.08", "ggx-beckmann-0.5", "ggx-roughdielectric-beckmann-0.15"):
        it, o = bc.items(name), oracle_all(oracle_lib, name)
        m = (it["wi_class"] == "grazing") & (it["wo_class"] == "wo=wi") & (np.abs(it["wi"][:, 2]) <= f32(1e-4))
        assert m.sum() >= 4
        assert not bits(o["eval"][m]).any() and not bits(o["epdf"][m]).any(), name


@pytest.mark.parametrize("name", bc.NAMES)
def test_flags(oracle_lib, name):
    """what the render derives from the material beside the values: ppgo_bsdf_flags / ppgo_bsdf_has_null against the plug-ins' getType()"""
    smooth, back, null = br.flags(_mat(name))
    assert oracle_all(oracle_lib, name)["flags"] == (1 if smooth else 0) | (2 if back else 0) | (4 if null else 0)


def measure():
    import __graft_entry__ as g
    lib = C.CDLL(g.oracle_library_path())
    print("%-50s %9s %9s  %-16s %-16s %s" % ("material", "LATTICE", "EDGE", "flagged LATTICE", "flagged EDGE", "K_ULPS"))
    for name in bc.NAMES:
        c, it = compare(lib, name), bc.items(name)
        w = [max(worst_remaining(c, it, e)[0].values()) for e in (False, True)]
        sh = [(c["eval_flagged"][it["is_edge"] == e].mean(), c["sample_flagged"][it["is_edge"] == e].mean()) for e in (False, True)]
        k = tuple(int(np.ceil(2 * v)) for v in w)
        print("%-50s %9.4g %9.4g  %.4f / %.4f  %.3f / %.3f   %r: %r," % (name, w[0], w[1], sh[0][0], sh[0][1], sh[1][0], sh[1][1], name, k), flush=True)


if __name__ == "__main__":
    measure()
