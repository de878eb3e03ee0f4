"""Emitter sampling and its MIS density on the CPU: the oracle's entry points ppgo_debug_sample_direct / ppgo_debug_pdf_direct (Scene::
sampleEmitterDirect up to the shadow ray; rayIntersect + Scene::pdfEmitterDirect) against the float64 restatement tests/emitter_ref.py,
item by item, at the cases tests/emitter_cases.py builds.  The device is held to the oracle bit for bit (tests/test_emitter_sampling_gpu.py),
so what fails here is what a device error of the same kind would trip.  Bounds, conditioning and what is left out: emitter_ref.py."""
import ctypes as C
import math

import numpy as np
import pytest

import emitter_cases as EC
import emitter_ref as ER
from conftest import make_oracle

f32 = np.float32


def _oracle(lib, desc):
    e = make_oracle(lib, budgetType="spp", budget=4)
    e.set_scene(desc)
    return e


def _sample(lib, desc, ref, ref_n, u):
    e = _oracle(lib, desc)
    got = e.debug_sample_direct_as(ref, ref_n, u)
    e.close()
    return got


def _on_emitter(name, got, R, ref, R_obj):
    """The sampled point ref + d dist of the record itself lies on the emitter: inside the chosen triangle, |p - c| = r on the sphere, on
    the bounding sphere's shell for the environment emitters — within the bound of a position, B scale + the restatement's conditioning.
    (Which triangle was chosen is discrete and the restatement's.)  Then the same point against the restatement's."""
    ok = R["sampled"] & ~R["skip"] & (R["kind"] != "other") & ((R["kind"] != "sphere") | (R["tol_n"] <= 1e-2)) & np.isfinite(R["d"]).all(1)
    ref = ref.astype(np.float64)
    p = ref + got["d"].astype(np.float64) * got["dist"].astype(np.float64)[:, None]
    bound = R["tol_dist"] + R["tol_d"] * R["dist"] + ER.B * (1 + np.abs(ref).max(1) + np.abs(p).max(1))
    worst = {}
    m = ok & (R["kind"] == "sphere")
    if m.any():
        sp = R_obj.spheres[0]
        c, r = np.asarray(sp["center"], np.float64), float(sp["radius"])
        off = np.abs(np.linalg.norm(p[m] - c, axis=1) - r)
        worst["|p - c| - r"] = float((off / bound[m]).max())
    m = ok & (R["kind"] == "env")
    if m.any():
        off = np.abs(np.linalg.norm(p[m] - R_obj.bs_c, axis=1) - R_obj.bs_r)
        worst["shell"] = float((off / bound[m]).max())
    m = ok & (R["kind"] == "mesh")
    if m.any():
        I = R_obj.I[R["extra"]["tri"][m]]
        p0, e1, e2 = R_obj.P[I[:, 0]], R_obj.P[I[:, 1]] - R_obj.P[I[:, 0]], R_obj.P[I[:, 2]] - R_obj.P[I[:, 0]]
        nn = np.cross(e1, e2)
        area2 = (nn * nn).sum(1)
        q = p[m] - p0
        bu, bv = (np.cross(q, e2) * nn).sum(1) / area2, (np.cross(e1, q) * nn).sum(1) / area2
        plane = np.abs((q * nn).sum(1)) / np.sqrt(area2)
        slack = bound[m] / np.minimum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))   # a position's bound in barycentric units
        outside = np.maximum(np.maximum(-bu, -bv), bu + bv - 1)
        worst["off the plane"] = float((plane / bound[m]).max())
        worst["outside the triangle"] = float(np.maximum(outside / slack, 0).max())
    far = np.abs(p - (ref + R["d"] * R["dist"][:, None])).max(1)
    worst["from the restatement's point"] = float((far[ok] / bound[ok]).max()) if ok.any() else 0.0
    print("   %s: the record's point on the emitter, %d items, largest distance / bound %s" % (name, int(ok.sum()), {k: round(v, 4) for k, v in worst.items()}))
    for k, v in worst.items():
        assert v <= 1.0, (name, k, v)


# ------------------------------------------------------------------------------------------------------------------------- the choice
def test_emitter_choice(oracle_lib):
    for name, desc, ref, ref_n, u in EC.choice_batches():
        got = _sample(oracle_lib, desc, ref, ref_n, u)
        R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
        EC.check_against_restatement(name, got, R)
        _on_emitter(name, got, R, ref, ER.EmitterRef(desc))
        empty = R["kind"] == "empty"
        assert (got["pdf"][empty] == 0).all() and (got["value"][empty] == 0).all() and (got["d"][empty] == 0).all()
        n_sel = len(R["kind"]) and len(np.unique(R["emitter"]))
        assert n_sel == len(ER.EmitterRef(desc).kind), name     # every entry of the table is chosen by some sample
        assert (R["em_pdf"] > 0).all()                          # no sample lands on an interval of width 0
        assert R["sx"].max() <= 1.0 and R["sx"].min() >= 0.0    # the re-used sample may reach 1


def test_pmf_sample_steps_over_an_empty_interval():
    """a cdf entry repeated (a triangle of area 0): samples on it, an ulp either side and at 0 never choose the empty interval"""
    cdf = np.array([0.0, 0.25, 0.25, 0.25, 0.75, 1.0], f32)
    v = EC.around(cdf)
    idx = ER.pmf_sample(cdf, v)
    assert ((cdf[idx + 1] - cdf[idx]) > 0).all()
    assert list(ER.pmf_sample(cdf, np.array([0.0, 0.25, np.nextafter(f32(0.25), f32(1)), 0.75, 1.0], f32))) == [0, 0, 3, 3, 4]
    lead = np.array([0.0, 0.0, 0.5, 1.0], f32)  # an empty first interval: a sample of exactly 0 steps over it
    assert list(ER.pmf_sample(lead, np.array([0.0, 1e-30, 0.5], f32))) == [1, 1, 1]


# --------------------------------------------------------------------------------------------------------------------------- the mesh
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (1e3, -2e3, 5e2)], ids=["origin", "translated"])
@pytest.mark.parametrize("normals", [False, True], ids=["face normal", "vertex normals"])
def test_mesh_emitter(oracle_lib, normals, shift):
    desc, ref, ref_n, u, cls = EC.mesh_batch(normals, shift)
    got = _sample(oracle_lib, desc, ref, ref_n, u)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    name = "mesh, %s, %s" % ("vertex normals" if normals else "face normal", "translated" if any(shift) else "at the origin")
    EC.check_against_restatement(name, got, R, cap_on=cls != "in plane")
    _on_emitter(name, got, R, ref, ER.EmitterRef(desc))
    tri = R["extra"]["tri"]
    assert set(np.unique(tri)) == {0, 1, 2, 4, 5} and (R["extra"]["area_width"] > 0).all()   # the triangle of area 0 is never chosen
    ok = ~R["skip"]
    print("   per class lit / dark:", {c: (int((ok & R["lit"] & (cls == c)).sum()), int((ok & ~R["lit"] & (cls == c)).sum())) for c in np.unique(cls)})
    for c in ("front", "front no refN"):
        assert (ok & R["lit"] & (cls == c)).sum() >= 500, c
    assert (ok & ~R["lit"] & (cls == "dark")).sum() >= 500
    b = R["extra"]["bary"]
    assert (b[:, 0] == 0).any() and (b[:, 0] >= 1 - 1e-3).any()   # a re-used sample of 0 and of (nearly) 1: the point on a vertex


def test_mesh_emitter_with_leading_empty_triangles(oracle_lib):
    desc, ref, ref_n, u = EC.leading_empty_batch()
    got = _sample(oracle_lib, desc, ref, ref_n, u)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    EC.check_against_restatement("mesh, two empty triangles first", got, R)
    assert set(np.unique(R["extra"]["tri"])) == {2, 3} and (R["extra"]["tri"][u[:, 1] == 0] == 2).all() and (u[:, 1] == 0).sum() >= 1000
    assert (R["extra"]["bary"][u[:, 1] == 0, 1] == 0).all()   # the re-used sample is 0 / width, not 0 / 0


# ------------------------------------------------------------------------------------------------------------------------- the sphere
def dark_threshold(got, R, ref_n):
    """of an unflipped sphere seen from afar (sinAlpha < 0.01) with refN = 0: the sinAlpha below which every sample has value 0, the
    largest at which one has, and the largest with a density of +inf"""
    s = R["extra"]["sin_alpha"]
    far = R["extra"]["cone"] & (s < 0.01) & (ref_n == 0).all(1)
    lit = (got["value"] != 0).any(1)
    inf = np.isinf(got["pdf"])
    return float(s[far & lit].min()), float(s[far & ~lit].max()), float(s[inf].max()) if inf.any() else 0.0


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flipped"])
def test_sphere_emitter(oracle_lib, flip):
    desc, ref, ref_n, u = EC.sphere_batch(flip)
    got = _sample(oracle_lib, desc, ref, ref_n, u)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    name = "sphere, %s" % ("flipped" if flip else "plain")
    EC.check_against_restatement(name, got, R, allow_inf_pdf=True)
    _on_emitter(name, got, R, ref, ER.EmitterRef(desc))
    s, cone = R["extra"]["sin_alpha"], R["extra"]["cone"]
    assert (cone & (s > 1 - 5e-4)).sum() >= 50 and (~cone & (s < 1 + 1e-3) & np.isfinite(s)).sum() >= 50   # both sides of the switch
    centre = ~np.isfinite(s)
    assert centre.sum() == 16
    if flip:   # from the centre every point of a flipped sphere is seen at distance r under cos 1: the density is 1 / (4 pi)
        seen = centre & (ref_n == 0).all(1)
        assert seen.sum() >= 4 and np.abs(got["pdf"][seen] - 0.25 * ER.INV_PI).max() <= ER.B and (got["value"][seen] > 0).all()
    else:
        assert (got["value"][centre] == 0).all() and (got["pdf"][centre] == 0).all()
    inf = np.isinf(got["pdf"])
    assert (got["value"][inf] == 0).all() and (s[inf] < 3e-4).all()   # the documented +inf density: 1 - sinAlpha^2 rounds to 1
    if not flip:
        assert inf.sum() >= 20
        all_dark_below, some_dark_up_to, inf_below = dark_threshold(got, R, ref_n)
        print("   sphere goes dark: every sample has value 0 below sinAlpha = %.3g, some up to %.3g; the density is +inf up to %.3g" % (
            all_dark_below, some_dark_up_to, inf_below))
        # 1 - sinAlpha^2 rounds to 1 exactly when sinAlpha^2 <= 2^-25: the density is +inf and the value 0 there, and only there
        edge = 2.0 ** -12.5
        assert inf_below <= edge * (1 + 1e-6) and all_dark_below >= edge * (1 - 1e-2)
        tiny = cone & (s < edge * (1 - 1e-6))
        assert (got["value"][tiny] == 0).all() and (np.isinf(got["pdf"][tiny]) | (got["pdf"][tiny] == 0)).all()   # (0: the facing tests failed)


# ------------------------------------------------------------------------------------------------------------ the constant environment
def test_constant_environment(oracle_lib):
    desc, ref, ref_n, u = EC.const_env_batch()
    got = _sample(oracle_lib, desc, ref, ref_n, u)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    EC.check_against_restatement("constant environment", got, R)
    _on_emitter("constant environment", got, R, ref, ER.EmitterRef(desc))
    outside = ~R["sampled"] & ~R["skip"]
    assert outside.sum() >= 200 and (got["pdf"][outside] == 0).all() and (got["dist"][outside] == 0).all()


# ------------------------------------------------------------------------------------------------------------- the environment map
MAPS = EC.envmap_maps()


@pytest.mark.parametrize("which", list(MAPS))
def test_environment_map(oracle_lib, which):
    rgb, to_world = MAPS[which]
    desc, ref, ref_n, u, ref_obj = EC.envmap_batch(rgb, to_world, oracle_lib)
    got = _sample(oracle_lib, desc, ref, ref_n, u)
    R = ref_obj.sample_direct(ref, ref_n, u)
    EC.check_against_restatement("envmap " + which, got, R)
    _on_emitter("envmap " + which, got, R, ref, ref_obj)
    ex = R["extra"]
    h, w = rgb.shape[:2]
    print("   tent offset: posX below 0 %d / above w - 1 %d, posY below 0 %d / above h - 1 %d; beyond a pole %d = %.4f of %d; failed samples %d" % (
        ex["x_below"].sum(), ex["x_above"].sum(), ex["y_below"].sum(), ex["y_above"].sum(), ex["pole_cross"].sum(), ex["pole_cross"].mean(), len(u), ex["fail"].sum()))
    if "black" not in which:
        assert ex["x_below"].any() and ex["x_above"].any() and ex["y_below"].any() and ex["y_above"].any() and not ex["fail"].any()
        assert ((ex["row_w"] > 0) & (ex["col_w"] > 0)).all()
    row_black = any(k in which for k in ("first row", "bright texel"))
    col_black = any(k in which for k in ("first column", "first row and column", "bright texel"))
    want_fail = [row_black or col_black, col_black, row_black]   # NAN_INPUTS: (0, 0), (0, .5), (.5, 0)
    assert list(ex["fail"][:3]) == want_fail
    assert (got["pdf"][ex["fail"]] == 0).all() and (got["value"][ex["fail"]] == 0).all() and (got["d"][ex["fail"]] == 0).all()


def test_zero_sample_in_front_of_a_black_row_or_column(oracle_lib):
    """The three inputs that gave a NaN direction and density (0 / 0 in sampleReuse): the failed sample, through both entry points"""
    m = EC.black_variants()["first row and column"]
    em = ppg_bindings_envmap(m)
    d, wgt, pdf = np.zeros((3, 3), f32), np.zeros((3, 3), f32), np.zeros(3, f32)
    from ppg_host.bindings import _fp
    assert oracle_lib.ppgo_envmap_sample(C.byref(em), 3, _fp(EC.NAN_INPUTS), _fp(d), _fp(wgt), _fp(pdf)) == 0
    assert (d == 0).all() and (wgt == 0).all() and (pdf == 0).all()
    desc = EC.envmap_scene(m)
    got = _sample(oracle_lib, desc, np.zeros((3, 3), f32), np.zeros((3, 3), f32), EC.NAN_INPUTS)
    for k in ("d", "n", "value", "sd"):
        assert (got[k] == 0).all(), k
    assert (got["pdf"] == 0).all() and (got["dist"] == 0).all() and (got["is_env"] == 1).all() and (got["em_pdf"] == 1).all()
    # a map whose first row and column are lit is not touched by the rule
    lit = _sample(oracle_lib, EC.envmap_scene(EC.random_map(8, 16)), np.zeros((3, 3), f32), np.zeros((3, 3), f32), EC.NAN_INPUTS)
    assert (lit["pdf"] > 0).all() and np.isfinite(lit["value"]).all()


def ppg_bindings_envmap(rgb):
    from ppg_host.bindings import EnvMap
    return EnvMap.from_dict(dict(rgb=rgb, scale=1.0, to_world=np.eye(3, dtype=f32).reshape(-1)))


@pytest.mark.parametrize("which", ["1x2", "3x5 rotated", "8x16", "32x64 sun", "8x16 black interior row and column"])
def test_environment_map_eval_and_density(oracle_lib, which):
    from ppg_host.bindings import EnvMap, _fp
    rgb, to_world = MAPS[which]
    tw = np.eye(3, dtype=f32).reshape(-1) if to_world is None else to_world
    E = ER.EnvMapRef(rgb, 1.5, tw, EC.sincos32(oracle_lib))
    dl = EC.envmap_directions(E)
    dw = (dl.astype(np.float64) @ E.R.T).astype(f32)
    em = EnvMap.from_dict(dict(rgb=rgb, scale=1.5, to_world=tw))
    val, pdf = np.zeros_like(dw), np.zeros(len(dw), f32)
    assert oracle_lib.ppgo_envmap_eval(C.byref(em), len(dw), _fp(dw), _fp(val), _fp(pdf)) == 0
    want_v, tol_v = E.eval(dw)
    want_p, tol_p = E.pdf_direction(dw.astype(np.float64) @ E.R)
    rv, rp = np.abs(val - want_v).max(1) / tol_v, np.abs(pdf - want_p) / np.maximum(tol_p, 1e-300)
    print("envmap %s: %d directions, largest error / bound: eval %.3f, pdfDirection %.3f" % (which, len(dw), rv.max(), rp.max()))
    assert np.isfinite(val).all() and np.isfinite(pdf).all()
    assert rv.max() <= 1 and rp.max() <= 1


# ------------------------------------------------------------------------------------------- the density of a BSDF-sampled ray, and MIS
def _rays(ref, d, maxt=np.inf):
    mint = ER.EPS * np.maximum(np.abs(ref).max(1), ER.EPS)
    return np.concatenate([ref, mint[:, None], d, np.full((len(ref), 1), maxt)], 1).astype(f32)


def mis_symmetry(name, engine, desc, R_obj, ref, ref_n, u, got, R, env=False, cap_on=None):
    """every lit sample's ray (ref, d) hits the same emitter and pdfEmitterDirect returns pdf * em_pdf within the bound; for the envmap the
    items whose tent offset crossed a pole are counted, not compared"""
    lit = (got["value"] != 0).any(1) & ~R["skip"] & (R["kind"] != "other") & (R["tol_n"] <= 1e-2) & np.isfinite(got["pdf"])
    rays = _rays(ref, got["d"])
    back = engine.debug_pdf_direct(rays, ref_n)
    P = R_obj.pdf_direct(rays, ref_n)
    # the ray meets something else first: the scene's own small triangle in front of the environment, or the near side of a sphere
    # whose far side was sampled from within 1e-4 of its surface (the switch class)
    with np.errstate(all="ignore"):
        occluded = ~P["skip"] & P["hit"] & ((P["emitter"] != R["emitter"]) | (np.abs(P["t"] - R["dist"]) > 1e-3 * (1 + R["dist"])))
    assert (occluded & lit).sum() <= 0.05 * max(1, lit.sum()), name
    lit = lit & ~occluded
    sel = lit & ~P["skip"]
    pole = R["extra"]["pole_cross"] if env and "pole_cross" in R["extra"] else np.zeros(len(u), bool)
    same = back["emitter"] == got["emitter"]
    assert same[sel].all(), (name, np.flatnonzero(sel & ~same)[:8])
    want = got["pdf"].astype(np.float64) * got["em_pdf"]
    with np.errstate(all="ignore"):
        tol = (R["tol_pdf"] + P["tol"]) * got["em_pdf"] + 4e-7 * want
        firm = (R["kind"] != "sphere") | (tol <= 1e-2 * want)   # (a sphere that subtends too little: emitter_ref.py)
        ratio = np.where(sel & ~pole & firm, np.abs(back["emitter_pdf"] - want) / tol, 0.0)
    share = float(pole[lit].mean()) if lit.any() else 0.0
    lit_ref = R["lit"] & ~R["skip"] & (R["kind"] != "other") & ~occluded
    assert share == (float(pole[lit_ref].mean()) if lit_ref.any() else 0.0), name   # the restatement's own count: the choice is discrete
    print("%s: MIS symmetry on %d lit samples (%d left out, %d of a sphere with a bound too loose, %d beyond a pole = %.4f), largest error / bound %.3f" % (
        name, int((sel & ~pole & firm).sum()), int((lit & ~sel).sum()), int((sel & ~firm).sum()), int((pole & lit).sum()), share, ratio.max()))
    assert ratio.max() <= 1.0, (name, int(ratio.argmax()), ratio.max())
    over = np.ones(len(u), bool) if cap_on is None else cap_on
    assert (lit & ~sel & over).sum() <= 0.02 * max(1, (lit & over).sum())
    return share


def test_mis_symmetry_mesh_and_sphere(oracle_lib):
    for name, (desc, ref, ref_n, u) in (("mesh", EC.mesh_batch(False, (0.0, 0.0, 0.0))[:4]), ("mesh, vertex normals", EC.mesh_batch(True, (0.0, 0.0, 0.0))[:4]),
                                        ("sphere", EC.sphere_batch(False)), ("sphere, flipped", EC.sphere_batch(True))):
        e = _oracle(oracle_lib, desc)
        got = e.debug_sample_direct_as(ref, ref_n, u)
        R_obj = ER.EmitterRef(desc)
        R = R_obj.sample_direct(ref, ref_n, u)
        off_surface = np.abs(np.linalg.norm(ref.astype(np.float64), axis=1) - 0.5) > 1e-3 if name.startswith("sphere") else None   # (not the switch class)
        mis_symmetry(name, e, desc, R_obj, ref, ref_n, u, got, R, cap_on=off_surface)
        e.close()


@pytest.mark.parametrize("which", ["1x2", "3x5", "8x16 rotated", "32x64 sun"])
def test_mis_symmetry_environment_map(oracle_lib, which):
    rgb, to_world = MAPS[which]
    desc, ref, ref_n, u, R_obj = EC.envmap_batch(rgb, to_world, oracle_lib)
    e = _oracle(oracle_lib, desc)
    got = e.debug_sample_direct_as(ref, ref_n, u)
    R = R_obj.sample_direct(ref, ref_n, u)
    share = mis_symmetry("envmap " + which, e, desc, R_obj, ref, ref_n, u, got, R, env=True)
    e.close()
    assert (share > 0) == bool(R["extra"]["pole_cross"].any())


def pdf_direct_batch(desc, R_obj, n=EC.N_BATCH, seed=71):
    """rays towards the emitters and past them, from points around the scene, with ref_n facing the ray, against it, across it and absent"""
    rng = np.random.default_rng(seed)
    ref = rng.uniform(-3, 3, (n, 3))
    target = rng.uniform(-1.6, 1.6, (n, 3)) * (1, 0.6, 0.3)
    if R_obj.n_area and R_obj.kind[0] == "mesh":   # three quarters of the rays at the emitter's triangles, largest first
        t = R_obj.I[R_obj.tris[0][rng.choice([0, 0, 0, 1, 1, 2, 4], 3 * n // 4)]]
        b = rng.dirichlet((1, 1, 1), 3 * n // 4)
        target[:3 * n // 4] = (R_obj.P[t] * b[:, :, None]).sum(1)
    d = EC.unit(target - ref)
    ref_n = EC.unit(d + rng.normal(0, 0.7, (n, 3)))
    k = n // 4
    ref_n[:k] = 0
    ref_n[k:2 * k] *= -1
    perp = EC.unit(np.cross(d[2 * k:2 * k + 64], rng.normal(size=(64, 3))))   # cos(refN) = 0 up to rounding
    ref_n[2 * k:2 * k + 64] = perp
    return _rays(ref.astype(f32).astype(np.float64), d), ref_n.astype(f32)


PDF_CASES = ["mesh", "mesh normals", "sphere", "sphere flipped", "constant", "envmap"]


def pdf_direct_case(which, lib):
    """-> the scene, its restatement, the rays and the normals of the vertices they left"""
    desc = dict(mesh=lambda: EC.mesh_scene(False), sphere=lambda: EC.sphere_scene(False), constant=EC.const_env_scene,
                envmap=lambda: EC.envmap_scene(EC.random_map(8, 16), EC.skew_rotation()))
    desc["mesh normals"] = lambda: EC.mesh_scene(True)
    desc["sphere flipped"] = lambda: EC.sphere_scene(True)
    desc = desc[which]()
    R_obj = ER.EmitterRef(desc, EC.sincos32(lib))
    rays, ref_n = pdf_direct_batch(desc, R_obj)
    if which.startswith("sphere"):   # the sample test's reference points, with rays through the sphere
        _, ref, _, _ = EC.sphere_batch(False)
        rays = _rays(ref.astype(np.float64), EC.unit(np.random.default_rng(5).normal(0, 0.3, ref.shape) * 0.5 - ref))
        rays = rays[np.isfinite(rays[:, 4:7]).all(1)]
        ref_n = ref_n[:len(rays)]
    return desc, R_obj, rays, ref_n


@pytest.mark.parametrize("which", PDF_CASES)
def test_pdf_direct(oracle_lib, which):
    desc, R_obj, rays, ref_n = pdf_direct_case(which, oracle_lib)
    e = _oracle(oracle_lib, desc)
    got = e.debug_pdf_direct(rays, ref_n)
    e.close()
    check_pdf_direct(which, got, R_obj, rays, ref_n)


def check_pdf_direct(which, got, R_obj, rays, ref_n):
    P = R_obj.pdf_direct(rays, ref_n)
    ok = ~P["skip"]
    assert ((got["prim"] >= 0) == P["hit"])[ok].all()
    assert (got["emitter"] == P["emitter"])[ok].all()
    assert np.isfinite(got["value"]).all() and not np.isnan(got["pdf_direct"]).any()
    if not which.startswith("sphere"):   # (the documented +inf of a sphere that subtends too little)
        assert np.isfinite(got["pdf_direct"]).all()
    lit_got, lit_ref = (got["value"] != 0).any(1), (P["value"] != 0).any(1)
    assert (lit_got == lit_ref)[ok].all()
    assert ((got["pdf_direct"] != 0) == (P["pdf_direct"] != 0))[ok].all()
    assert (got["pdf_direct"][ok & ~lit_ref] == 0).all()
    norm = float(R_obj.sel_norm)
    with np.errstate(all="ignore"):
        firm = (P["tol"] <= 1e-2 * P["pdf_direct"]) if which.startswith("sphere") else np.ones(len(rays), bool)   # (a sphere that subtends too little)
        sel = ok & (P["pdf_direct"] != 0) & firm
        ratio = np.where(sel, np.abs(got["pdf_direct"] - P["pdf_direct"]) / P["tol"], 0.0)
        rv = np.where(ok[:, None] & lit_ref[:, None], np.abs(got["value"] - P["value"]) / (ER.B * np.abs(P["value"]).max(1, keepdims=True) + 1e-30), 0.0)
    assert (got["emitter_pdf"] == (got["pdf_direct"] * f32(norm)).astype(f32)).all()
    print("pdf_direct %s: %d rays, hits %d, emitters seen %d, densities compared %d, left out %d, bound too loose %d; largest error / bound: density %.3f, value %.3f" % (
        which, len(rays), int(P["hit"].sum()), int(lit_ref.sum()), int(sel.sum()), int(P["skip"].sum()), int((ok & (P["pdf_direct"] != 0) & ~firm).sum()),
        ratio.max(), rv.max()))
    on_surface = np.abs(np.linalg.norm(rays[:, :3], axis=1) - 0.5) < 1e-3 if which.startswith("sphere") else np.zeros(len(rays), bool)   # the switch class: the near root is at mint
    assert (P["skip"] & ~on_surface).sum() <= 0.02 * len(rays) and sel.sum() >= 500
    if which == "envmap":
        E = R_obj.envmap
        want, tol = E.eval(rays[:, 4:7])
        rv = np.where(ok[:, None] & lit_ref[:, None], np.abs(got["value"] - want) / tol[:, None], 0.0)
    assert ratio.max() <= 1 and rv.max() <= 1
    if which == "constant":  # cos(refN) positive, zero (a rounding either side), negative, and no refN
        cos = (rays[:, 4:7].astype(np.float64) * ref_n).sum(1)
        none = (ref_n == 0).all(1)
        out = ok & ~P["hit"] & (P["emitter"] >= 0)   # the ray leaves the scene inside the bounding sphere
        assert (got["pdf_direct"][none & out] == f32(ER.INV_PI * 0.25)).all() and (got["pdf_direct"][~none & (cos < -1e-4) & out] == 0).all()
        assert (np.abs(cos[~none]) < 1e-6).sum() >= 32 and (got["pdf_direct"][~none & (cos > 1e-4) & out] > 0).all()
        assert (none & out).sum() >= 100 and (~none & (cos < -1e-4) & out).sum() >= 100


# ------------------------------------------------------------------------------------------------------------ the estimator integrates
def estimator_cases(lib):
    """per emitter kind: (name, desc, ref point, ref normal, the integral of radiance over the emitter's solid angle by quadrature)"""
    out = []
    desc = EC.mesh_scene(False)
    R = ER.EmitterRef(desc)
    pt = np.array([0.2, 0.4, 1.5])
    quad = sum(ER.triangle_quadrature(pt, *[R.P[i] for i in R.I[t]], R.radiance[0]) for t in R.tris[0] if t != 3)
    out.append(("mesh", desc, pt, np.zeros(3), quad))
    desc = EC.sphere_scene(False)
    pt = np.array([0.9, -0.4, 1.2])
    cos_a = math.sqrt(1 - (0.5 / np.linalg.norm(pt.astype(f32).astype(np.float64))) ** 2)
    out.append(("sphere", desc, pt, np.zeros(3), np.array([2.0, 3.0, 4.0]) * 2 * math.pi * (1 - cos_a)))
    desc = EC.const_env_scene()
    out.append(("constant environment", desc, np.array([0.1, 0.2, 0.3]), np.array([0.0, 0.6, 0.8]), np.array([1.0, 2.0, 3.0]) * 2 * math.pi))
    rgb = EC.sun_map()
    desc = EC.envmap_scene(rgb, EC.skew_rotation())
    E = ER.EnvMapRef(rgb, 1.5, EC.skew_rotation(), EC.sincos32(lib))
    nt, npp = 720, 1440
    th, ph = (np.arange(nt) + 0.5) / nt * math.pi, (np.arange(npp) + 0.5) / npp * 2 * math.pi
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    dl = np.stack([np.sin(TH) * np.sin(PH), np.cos(TH), -np.sin(TH) * np.cos(PH)], -1).reshape(-1, 3)
    val, _ = E.eval(dl @ E.R.T)
    out.append(("environment map", desc, np.array([0.1, 0.2, 0.3]), np.zeros(3), (val * (np.sin(TH).reshape(-1) * (math.pi / nt) * (2 * math.pi / npp))[:, None]).sum(0)))
    return out


def check_estimator(name, sample, desc, pt, nrm, quad, lib):
    """mean(value) over 16 384 uniform samples = the quadrature, within 4 standard errors of the restatement's own samples"""
    n = 16384
    u = np.minimum(np.random.default_rng(81).uniform(0, 1, (n, 2)), EC.TOP).astype(f32)
    ref, ref_n = np.tile(pt.astype(f32), (n, 1)), np.tile(nrm.astype(f32), (n, 1))
    got = sample(desc, ref, ref_n, u)
    R = ER.EmitterRef(desc, EC.sincos32(lib)).sample_direct(ref, ref_n, u)
    vals = np.where(np.isfinite(R["value"]), R["value"], 0.0)
    se = vals.std(0) / math.sqrt(n)
    mean = got["value"].astype(np.float64).mean(0)
    dev = np.abs(mean - quad) / np.maximum(se, 1e-9 * np.abs(quad))
    print("estimator %s: mean %s, quadrature %s, standard error %s, deviation / standard error %s; deviation / (4 standard errors + the float32 term B |quadrature|) %s" % (
        name, mean, quad, se, np.round(dev, 2), np.round(np.abs(mean - quad) / (4 * se + ER.B * np.abs(quad)), 3)))
    assert (np.abs(mean - quad) <= 4 * se + ER.B * np.abs(quad)).all(), name   # (the cone's value is a constant without spread: float32 remains)


def test_the_estimator_integrates(oracle_lib):
    for name, desc, pt, nrm, quad in estimator_cases(oracle_lib):
        check_estimator(name, lambda d, a, b, c: _sample(oracle_lib, d, a, b, c), desc, pt, nrm, quad, oracle_lib)


# ------------------------------------------------------------------------------------------------ escaped rays at the named directions
ESCAPE_MAPS = ["1x2", "3x5 rotated", "8x16", "32x64 sun"]


def envmap_escape_case(which, lib):
    """EC.envmap_directions — the lat-long grid, +-y exactly, the seam and an ulp either side, texel centre lines and an ulp either side —
    rotated to world, as rays that leave the scene from the bounding sphere's centre, without a refN"""
    rgb, to_world = MAPS[which]
    desc = EC.envmap_scene(rgb, to_world)
    R_obj = ER.EmitterRef(desc, EC.sincos32(lib))
    E = R_obj.envmap
    dl = EC.envmap_directions(E)
    dw = (dl.astype(np.float64) @ E.R.T).astype(f32)
    rays = _rays(np.tile(R_obj.bs_c.astype(f32).astype(np.float64), (len(dw), 1)), dw.astype(np.float64))
    return desc, R_obj, rays, np.zeros((len(dw), 3), f32)


def check_envmap_escape(which, got, R_obj, rays):
    """envmap_eval and envmap_pdf_direction of the escaped rays against the restatement's eval / pdf_direction within their bounds"""
    E = R_obj.envmap
    P = R_obj.pdf_direct(rays, np.zeros((len(rays), 3), f32))
    out = ~P["hit"] & ~P["skip"]
    assert out.sum() >= 0.95 * len(rays) and (got["prim"][out] == -1).all() and (got["emitter"][out] == R_obj.n_sel - 1).all()
    assert np.isfinite(got["value"]).all() and np.isfinite(got["pdf_direct"]).all()
    d = rays[:, 4:7].astype(np.float64)
    want_v, tol_v = E.eval(d)
    want_p, tol_p = E.pdf_direction(d @ E.R)
    lit = (want_v != 0).any(1)
    rv = np.where(out, np.abs(got["value"] - want_v).max(1) / tol_v, 0.0)
    rp = np.where(out & lit & (got["value"] != 0).any(1), np.abs(got["pdf_direct"] - want_p) / np.maximum(tol_p, 1e-300), 0.0)
    assert (got["pdf_direct"][out & ~(got["value"] != 0).any(1)] == 0).all()   # the density is asked for a lit direction only
    assert (got["emitter_pdf"] == (got["pdf_direct"] * f32(R_obj.sel_norm)).astype(f32)).all()
    print("envmap %s: %d escaped rays at the named directions (%d occluded by the scene's triangle), largest error / bound: radiance %.3f, density %.3f" % (
        which, int(out.sum()), int(P["hit"].sum()), rv.max(), rp.max()))
    assert rv.max() <= 1 and rp.max() <= 1


@pytest.mark.parametrize("which", ESCAPE_MAPS)
def test_environment_map_escaped_rays(oracle_lib, which):
    desc, R_obj, rays, ref_n = envmap_escape_case(which, oracle_lib)
    e = _oracle(oracle_lib, desc)
    got = e.debug_pdf_direct(rays, ref_n)
    e.close()
    check_envmap_escape(which, got, R_obj, rays)


# ------------------------------------------------------------------------------------------------------------------- shares and layout
POLE_COUNTS = {"1x1": 4028, "1x2": 4028, "2x1": 2038, "3x5": 893, "8x16": 160, "32x64 sun": 6}   # of 16 384: DESIGN.md's shares


def test_pole_crossing_shares(oracle_lib):
    """how many of 16 384 uniform samples (seed 7) the tent offset puts beyond a pole, per map: the figures DESIGN.md quotes.  The choice
    of row and column is discrete, so the counts are exact; the oracle's samples at the same inputs agree with the restatement."""
    u = np.minimum(np.random.default_rng(7).uniform(0, 1, (16384, 2)), EC.TOP).astype(f32)
    for which, count in POLE_COUNTS.items():
        rgb, _ = MAPS[which]
        desc = EC.envmap_scene(rgb)
        R_obj = ER.EmitterRef(desc, EC.sincos32(oracle_lib))
        ref = np.tile(R_obj.bs_c.astype(f32), (len(u), 1))
        R = R_obj.sample_direct(ref, np.zeros_like(ref), u)
        got = _sample(oracle_lib, desc, ref, np.zeros_like(ref), u)
        EC.check_against_restatement("envmap %s, uniform samples" % which, got, R)
        pole = R["extra"]["pole_cross"]
        print("   envmap %s: beyond a pole %d of %d = %.2f %%" % (which, pole.sum(), len(u), 100 * pole.mean()))
        assert pole.sum() == count, (which, int(pole.sum()))


def test_new_records_have_the_layout_of_the_header(tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    from ppg_host import bindings as b
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppg_testhooks.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(struct ppg_debug_direct), sizeof(struct ppg_debug_direct_ex), sizeof(struct ppg_debug_pdf), offsetof(struct ppg_debug_direct_ex, value), '
                   'offsetof(struct ppg_debug_direct_ex, sd), offsetof(struct ppg_debug_direct_ex, sdist), offsetof(struct ppg_debug_direct_ex, is_delta), '
                   'offsetof(struct ppg_debug_pdf, value), offsetof(struct ppg_debug_pdf, emitter_pdf)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    X, Q = b.DebugDirectEx, b.DebugPdf
    assert got == [C.sizeof(b.DebugDirect), C.sizeof(X), C.sizeof(Q), X.value.offset, X.sd.offset, X.sdist.offset, X.is_delta.offset, Q.value.offset, Q.emitter_pdf.offset]
    assert got[:3] == [64, 80, 32] and b.DEBUG_DIRECT_EX_DTYPE.itemsize == 80 and b.DEBUG_PDF_DTYPE.itemsize == 32
    for name in b.DEBUG_DIRECT_DTYPE.names[:-1]:   # the extended record starts with the plain one
        assert b.DEBUG_DIRECT_DTYPE.fields[name][1] == b.DEBUG_DIRECT_EX_DTYPE.fields[name][1], name


def test_samples_outside_the_unit_square_are_refused(oracle_lib):
    import ppg_host
    e = _oracle(oracle_lib, EC.mesh_scene(False))
    z = np.zeros((1, 3), f32)
    for bad in ((1.0000001, 0.5), (0.5, 1.5), (-1e-9, 0.5), (0.5, np.nan)):
        with pytest.raises(ppg_host.PPGError, match="outside"):
            e.debug_sample_direct_as(z, z, np.array([bad], f32))
    assert e.debug_sample_direct_as(z, z, np.array([[1.0, 1.0]], f32))["emitter"][0] == 0   # 1 itself is inside: the re-used sample may reach it
    e.close()
