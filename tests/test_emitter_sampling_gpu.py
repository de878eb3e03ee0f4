"""Emitter sampling and its MIS density on the device, item by item (include/ppg_testhooks.h ppg_debug_sample_direct_as, ppg_debug_pdf_direct):

  * device = oracle, bit for bit, on every field of every item — the project's contract for everything the oracle knows — for the copy of
    emitter_sample_direct / emitter_pdf_direct in every kernel family's module and for both FULL settings of the base family;
  * device = the float64 restatement (tests/emitter_ref.py) within its bounds, on the items it does not leave out;
  * the properties that need neither: the sampled point lies on the emitter, MIS symmetry, the estimator integrates;
  * for selection tables the oracle refuses (delta emitters, a disk, a cylinder): the emitter index and its probability exactly.

The scenes, batches and the checks themselves are those of the CPU file (tests/emitter_cases.py, tests/test_emitter_sampling.py)."""
import numpy as np
import pytest

import emitter_cases as EC
import emitter_ref as ER
import test_emitter_sampling as T
from conftest import make_oracle

f32 = np.float32
pytestmark = pytest.mark.gpu
FAMILIES = 6  # PPG_FAMILIES (csrc/ppg_device.h)


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def _device(desc):
    e = hip(budgetType="spp", budget=4)
    e.set_scene(desc)
    return e


def _variants(e, ref, ref_n, u, plain):
    """the record of every instantiation that can read the scene: (family, full) -> record.  `plain`: the scene's render is not FULL, so
    the base family's full = 0 exists for it; for every other scene that call must be refused."""
    import ppg_host
    out = {(-1, -1): e.debug_sample_direct_as(ref, ref_n, u)}
    for fam in range(FAMILIES):
        out[(fam, 1)] = e.debug_sample_direct_as(ref, ref_n, u, family=fam, full=1)
    if plain:
        out[(0, 0)] = e.debug_sample_direct_as(ref, ref_n, u, family=0, full=0)
    else:
        with pytest.raises(ppg_host.PPGError, match="FULL"):
            e.debug_sample_direct_as(ref[:1], ref_n[:1], u[:1], family=0, full=0)
    out[("shapes hook", 1)] = e.debug_sample_direct(ref, ref_n, u)
    return out


def _equal_oracle(name, oracle_lib, desc, ref, ref_n, u, plain):
    """every instantiation against the oracle, byte for byte -> the record"""
    want = T._sample(oracle_lib, desc, ref, ref_n, u)
    e = _device(desc)
    got = _variants(e, ref, ref_n, u, plain)
    e.close()
    for key, rec in got.items():
        if key[0] == "shapes hook":   # the plain 64-byte record: the extended one's first fields, the padding 0
            for k in rec.dtype.names[:-1]:
                assert np.ascontiguousarray(rec[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (name, key, k)
            assert (rec["_pad"] == 0).all()
            continue
        assert EC.bits_equal(rec, want), (name, key, EC.first_difference(rec, want))
    print("%s: %d instantiations equal the oracle bit for bit on %d items" % (name, len(got), len(u)))
    return want


def test_emitter_choice(oracle_lib):
    for name, desc, ref, ref_n, u in EC.choice_batches():
        got = _equal_oracle(name, oracle_lib, desc, ref, ref_n, u, plain=desc.environment is None)
        R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
        EC.check_against_restatement(name, got, R)
        T._on_emitter(name, got, R, ref, ER.EmitterRef(desc))


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (1e3, -2e3, 5e2)], ids=["origin", "translated"])
@pytest.mark.parametrize("normals", [False, True], ids=["face normal", "vertex normals"])
def test_mesh_emitter(oracle_lib, normals, shift):
    desc, ref, ref_n, u, cls = EC.mesh_batch(normals, shift)
    name = "mesh, %s, %s" % ("vertex normals" if normals else "face normal", "translated" if any(shift) else "at the origin")
    got = _equal_oracle(name, oracle_lib, desc, ref, ref_n, u, plain=True)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    EC.check_against_restatement(name, got, R, cap_on=cls != "in plane")
    T._on_emitter(name, got, R, ref, ER.EmitterRef(desc))


def test_mesh_emitter_with_leading_empty_triangles(oracle_lib):
    desc, ref, ref_n, u = EC.leading_empty_batch()
    got = _equal_oracle("mesh, two empty triangles first", oracle_lib, desc, ref, ref_n, u, plain=True)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    EC.check_against_restatement("mesh, two empty triangles first", got, R)
    assert (R["extra"]["tri"][u[:, 1] == 0] == 2).all()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flipped"])
def test_sphere_emitter(oracle_lib, flip):
    desc, ref, ref_n, u = EC.sphere_batch(flip)
    name = "sphere, %s" % ("flipped" if flip else "plain")
    got = _equal_oracle(name, oracle_lib, desc, ref, ref_n, u, plain=False)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    EC.check_against_restatement(name, got, R, allow_inf_pdf=True)
    T._on_emitter(name, got, R, ref, ER.EmitterRef(desc))
    if not flip:
        all_dark_below, some_dark_up_to, inf_below = T.dark_threshold(got, R, ref_n)
        print("   sphere goes dark: every sample has value 0 below sinAlpha = %.3g, some up to %.3g; the density is +inf up to %.3g" % (
            all_dark_below, some_dark_up_to, inf_below))
        assert inf_below <= 2.0 ** -12.5 * (1 + 1e-6)


def test_constant_environment(oracle_lib):
    desc, ref, ref_n, u = EC.const_env_batch()
    got = _equal_oracle("constant environment", oracle_lib, desc, ref, ref_n, u, plain=False)
    R = ER.EmitterRef(desc).sample_direct(ref, ref_n, u)
    EC.check_against_restatement("constant environment", got, R)
    T._on_emitter("constant environment", got, R, ref, ER.EmitterRef(desc))


@pytest.mark.parametrize("which", list(T.MAPS))
def test_environment_map(oracle_lib, which):
    rgb, to_world = T.MAPS[which]
    desc, ref, ref_n, u, ref_obj = EC.envmap_batch(rgb, to_world, oracle_lib)
    got = _equal_oracle("envmap " + which, oracle_lib, desc, ref, ref_n, u, plain=False)
    R = ref_obj.sample_direct(ref, ref_n, u)
    EC.check_against_restatement("envmap " + which, got, R)
    T._on_emitter("envmap " + which, got, R, ref, ref_obj)
    fail = R["extra"]["fail"]
    assert (got["pdf"][fail] == 0).all() and (got["value"][fail] == 0).all() and (got["d"][fail] == 0).all()


def test_zero_sample_in_front_of_a_black_row_or_column(oracle_lib):
    """the three inputs that gave NaN (0 / 0 in envmap_sample_reuse) return the failed sample in every instantiation"""
    desc = EC.envmap_scene(EC.black_variants()["first row and column"])
    z = np.zeros((3, 3), f32)
    got = _equal_oracle("black first row and column", oracle_lib, desc, z, z, EC.NAN_INPUTS, plain=False)
    for k in ("d", "n", "value", "sd"):
        assert (got[k] == 0).all(), k
    assert (got["pdf"] == 0).all() and (got["dist"] == 0).all() and (got["is_env"] == 1).all() and (got["em_pdf"] == 1).all()


# ------------------------------------------------------------------------------------------------------------- the density and MIS
def _pdf_fields_equal(name, rec, want, n_tri):
    """every field but prim byte for byte; prim (leaf order on the device, scene order in the oracle) where the two orders cannot differ"""
    for k in ("emitter", "value", "pdf_direct", "emitter_pdf"):
        a, b = np.ascontiguousarray(rec[k]), np.ascontiguousarray(want[k])
        assert a.tobytes() == b.tobytes(), (name, k, int(np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1))[0]))
    assert ((rec["prim"] >= 0) == (want["prim"] >= 0)).all() and ((rec["prim"] >= n_tri) == (want["prim"] >= n_tri)).all(), name
    sph = want["prim"] >= n_tri
    assert (rec["prim"][sph] == want["prim"][sph]).all(), name


@pytest.mark.parametrize("which", T.PDF_CASES)
def test_pdf_direct(oracle_lib, which):
    import ppg_host
    desc, R_obj, rays, ref_n = T.pdf_direct_case(which, oracle_lib)
    o = T._oracle(oracle_lib, desc)
    want = o.debug_pdf_direct(rays, ref_n)
    o.close()
    e = _device(desc)
    n_tri = len(np.asarray(desc.indices).reshape(-1, 3))
    for fam in [-1] + list(range(FAMILIES)):
        _pdf_fields_equal("pdf_direct %s, family %d" % (which, fam), e.debug_pdf_direct(rays, ref_n, family=fam), want, n_tri)
    with pytest.raises(ppg_host.PPGError):
        e.debug_pdf_direct(rays[:1], ref_n[:1], family=FAMILIES)
    got = e.debug_pdf_direct(rays, ref_n)
    e.close()
    T.check_pdf_direct(which, got, R_obj, rays, ref_n)


@pytest.mark.parametrize("which", T.ESCAPE_MAPS)
def test_environment_map_escaped_rays(oracle_lib, which):
    """envmap_eval and envmap_pdf_direction of every family at the directions that can go wrong — the poles (the PPG_EPSILON clamp at sin
    theta = 0), the seam of atan2 and an ulp either side, texel centre lines and an ulp either side, a lat-long grid — as rays that
    leave the scene: the oracle's record bit for bit, and the restatement's eval / pdf_direction within their bounds"""
    desc, R_obj, rays, ref_n = T.envmap_escape_case(which, oracle_lib)
    o = T._oracle(oracle_lib, desc)
    want = o.debug_pdf_direct(rays, ref_n)
    o.close()
    e = _device(desc)
    n_tri = len(np.asarray(desc.indices).reshape(-1, 3))
    for fam in [-1] + list(range(FAMILIES)):
        _pdf_fields_equal("envmap %s escaped rays, family %d" % (which, fam), e.debug_pdf_direct(rays, ref_n, family=fam), want, n_tri)
    got = e.debug_pdf_direct(rays, ref_n)
    e.close()
    T.check_envmap_escape(which, got, R_obj, rays)


def test_samples_outside_the_unit_square_are_refused():
    import ppg_host
    e = _device(EC.mesh_scene(False))
    z = np.zeros((1, 3), f32)
    for bad in ((1.0000001, 0.5), (0.5, 1.5), (-1e-9, 0.5), (0.5, np.nan)):
        with pytest.raises(ppg_host.PPGError, match="outside"):
            e.debug_sample_direct_as(z, z, np.array([bad], f32))
        with pytest.raises(ppg_host.PPGError, match="outside"):
            e.debug_sample_direct(z, z, np.array([bad], f32))
    assert e.debug_sample_direct_as(z, z, np.array([[1.0, 1.0]], f32))["emitter"][0] == 0
    e.close()


def test_mis_symmetry(oracle_lib):
    cases = [("mesh", EC.mesh_batch(False, (0.0, 0.0, 0.0))[:4], None), ("mesh, vertex normals", EC.mesh_batch(True, (0.0, 0.0, 0.0))[:4], None),
             ("sphere", EC.sphere_batch(False), None), ("sphere, flipped", EC.sphere_batch(True), None)]
    for which in ("1x2", "3x5", "8x16 rotated", "32x64 sun"):
        rgb, to_world = T.MAPS[which]
        desc, ref, ref_n, u, R_obj = EC.envmap_batch(rgb, to_world, oracle_lib)
        cases.append(("envmap " + which, (desc, ref, ref_n, u), R_obj))
    for name, (desc, ref, ref_n, u), R_obj in cases:
        e = _device(desc)
        got = e.debug_sample_direct_as(ref, ref_n, u)
        R_obj = R_obj or ER.EmitterRef(desc)
        R = R_obj.sample_direct(ref, ref_n, u)
        off_surface = np.abs(np.linalg.norm(ref.astype(np.float64), axis=1) - 0.5) > 1e-3 if name.startswith("sphere") else None
        T.mis_symmetry(name, e, desc, R_obj, ref, ref_n, u, got, R, env=name.startswith("envmap"), cap_on=off_surface)
        e.close()


def test_the_estimator_integrates(oracle_lib):
    def sample(desc, ref, ref_n, u):
        e = _device(desc)
        got = e.debug_sample_direct_as(ref, ref_n, u)
        e.close()
        return got
    for name, desc, pt, nrm, quad in T.estimator_cases(oracle_lib):
        T.check_estimator(name, sample, desc, pt, nrm, quad, oracle_lib)


# ------------------------------------------------------------------------------------------------- what the oracle does not know
def test_choice_among_delta_emitters_and_shapes():
    """a selection table of a mesh emitter, a disk, a cylinder, two delta emitters and the environment: the oracle refuses the scene; the
    emitter index and its probability against the restatement's float32 table, exactly, and the kinds' flags"""
    desc = EC.choice_scene(1, None, env=True)
    desc.emitters = [dict(radiance=(1.0, 2.0, 0.5)), dict(radiance=(2.0, 1.0, 1.0)), dict(radiance=(0.5, 0.5, 3.0))]
    desc.shapes = [dict(type="disk", to_world=[0.3, 0, 0, 2.0, 0, 0.3, 0, 0.5, 0, 0, 0.3, 0.2], material=0, emitter=1),
                   dict(type="cylinder", to_world=[1, 0, 0, -2.0, 0, 1, 0, 0.5, 0, 0, 1, 0.0], radius=0.2, length=0.7, material=0, emitter=2)]
    desc.delta_emitters = [dict(type="point", intensity=(3.0, 2.0, 1.0), position=(0.5, 1.5, 1.0)),
                           dict(type="directional", intensity=(1.0, 1.0, 1.0), direction=(0.0, -1.0, 0.0))]
    R_obj = ER.EmitterRef(desc)
    assert R_obj.n_sel == 6 and R_obj.kind == ["mesh", "other", "other", "other", "other", "env"]
    rng = np.random.default_rng(91)
    u, _ = EC.grid_with(EC.around(R_obj.sel_cdf), np.array([0.0, 0.3, EC.TOP], f32), EC.N_BATCH, rng)
    ref = rng.uniform(-1, 1, (EC.N_BATCH, 3)).astype(f32) + f32([0, 0, 1.5])
    ref_n = np.zeros((EC.N_BATCH, 3), f32)
    e = _device(desc)
    recs = {fam: e.debug_sample_direct_as(ref, ref_n, u, family=fam) for fam in (-1, 1, 2, 3, 4, 5)}
    import ppg_host
    with pytest.raises(ppg_host.PPGError, match="kernel family"):
        e.debug_sample_direct_as(ref[:1], ref_n[:1], u[:1], family=0, full=1)   # the base family knows no disks and cylinders
    with pytest.raises(ppg_host.PPGError, match="base family"):
        e.debug_sample_direct_as(ref[:1], ref_n[:1], u[:1], family=2, full=0)
    e.close()
    R = R_obj.sample_direct(ref, ref_n, u)
    for fam, got in recs.items():
        assert EC.bits_equal(got, recs[-1]), (fam, EC.first_difference(got, recs[-1]))
    got = recs[-1]
    assert (got["emitter"] == R["emitter"]).all() and (got["em_pdf"] == R["em_pdf"]).all()
    assert (got["is_delta"] == ((R["emitter"] == 3) | (R["emitter"] == 4))).all() and (got["is_env"] == (R["emitter"] == 5)).all()
    assert np.isfinite(got["value"]).all() and np.isfinite(got["pdf"]).all()
    print("choice among 6 entries (mesh, disk, cylinder, point, directional, environment): chosen %s, %d items, exact" % (
        np.bincount(got["emitter"], minlength=6).tolist(), len(u)))
    assert (np.bincount(got["emitter"], minlength=6) > 0).all()
    # (no continuous comparison here: the restatement knows neither the shapes nor what they add to the scene's box and bounding sphere)
