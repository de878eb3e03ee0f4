"""Pin (1) of the oracle: the known answers of SURVEY.md §8(c) / Appendix A (obtained there by compiling
guided_path.cpp:33-1007) and the algebraic identities of Appendix A."""
import ctypes as C

import numpy as np

import ref_sdtree as R  # the reference's own classes where oracle/_ref exists: a second opinion on the known answers below


def test_fresh_reset_is_depth4_85_nodes(oracle_lib):
    # every reference log: "Depth = [4, 4, 4] ... Node count = [85, 85, 85]" at iteration 0 (GP:456-514, rho = 0.01)
    nn, d, pdf = C.c_uint32(), C.c_int32(), C.c_float()
    assert oracle_lib.ppgo_ka_fresh_reset(C.c_float(0.01), C.byref(nn), C.byref(d), C.byref(pdf)) == 0
    assert (nn.value, d.value) == (85, 4)
    assert abs(pdf.value - 0.0795775) < 1e-7  # 1 / (4 pi): no data yet (GP:415-418)


def test_refine_known_answer(oracle_lib):
    # refine(W = 4 349 763, thr = 16 970) -> 512 leaves (GP:957-998)
    nl, nn = C.c_uint32(), C.c_uint32()
    assert oracle_lib.ppgo_ka_refine(C.c_float(4349763), C.c_uint64(16970), C.byref(nl), C.byref(nn)) == 0
    assert (nl.value, nn.value) == (512, 1023)
    oracle_lib.ppgo_ka_refine(C.c_float(16970), C.c_uint64(16970), C.byref(nl), C.byref(nn))
    assert nl.value == 1  # split only if weight > threshold (GP:953-955)
    oracle_lib.ppgo_ka_refine(C.c_float(16971), C.c_uint64(16970), C.byref(nl), C.byref(nn))
    assert nl.value == 2
    ref = R.second_opinion()  # the same three answers from STree::refine of the reference's text
    if ref is not None:
        for W, leaves in ((4349763, 512), (16970, 1), (16971, 2)):
            one = {"offset": np.zeros(1, np.uint64), "num_nodes": np.ones(1, np.uint32), "max_depth": np.zeros(1, np.int32), "sum": np.zeros(1, np.float32),
                   "stat_weight": np.float32([W]), "node_sums": np.zeros((1, 4), np.float32), "node_children": np.zeros((1, 4), np.uint16)}
            ref.load({"axis": np.zeros(1, np.int32), "children": np.zeros((1, 2), np.uint32), "theta": np.zeros(1, np.float32),
                      "aabb_min": np.zeros(3, np.float32), "aabb_max": np.ones(3, np.float32), "sampling": one, "building": one})
            ref.refine_reset(16970, -1, 20, 0.01)
            assert ref.read()["n_leaves"] == leaves


def test_adam_known_answer(oracle_lib):
    # 10 identical KL records -> fraction 0.512494385 (GP:672-697, 85-109).
    # ppg_detmath's exp/powi differ from libm by <= 1 ulp, hence the 2e-7 tolerance.
    fr = C.c_float()
    oracle_lib.ppgo_ka_adam(10, C.c_float(.5), C.c_float(.2), C.c_float(.3), C.c_float(.1), C.c_float(1), 1, C.byref(fr))
    assert abs(fr.value - 0.512494385) < 2e-7
    fr_ten = fr.value
    oracle_lib.ppgo_ka_adam(1, C.c_float(.5), C.c_float(.2), C.c_float(.3), C.c_float(.1), C.c_float(1), 1, C.byref(fr))
    assert fr.value == 0.5  # batchAccumulation 1 > batchSize 1 is false: no step yet (GP:89)
    ref = R.second_opinion()  # the reference's own optimizeBsdfSamplingFraction / AdamOptimizer with libm's exp and pow
    if ref is not None:
        st = ref.adam_replay(np.zeros(6, np.uint32), np.tile(np.float32([.5, .2, .3, .1, 1]), (10, 1)), 1)
        assert st[1] == 5 and abs(1 / (1 + np.exp(-float(st[:1].view(np.float32)[0]))) - 0.512494385) < 1e-7
        assert abs(1 / (1 + np.exp(-float(st[:1].view(np.float32)[0]))) - fr_ten) < 2e-7
        st = ref.adam_replay(np.zeros(6, np.uint32), np.float32([[.5, .2, .3, .1, 1]]), 1)
        assert st[0] == 0 and st[1] == 0


def test_canonical_direction_maps(oracle_lib):
    oracle_lib.ppgo_canonical_to_dir.restype = None
    oracle_lib.ppgo_dir_to_canonical.restype = None
    rng = np.random.RandomState(3)
    for _ in range(2000):
        x, y = rng.rand(2).astype(np.float32)
        d = (C.c_float * 3)()
        oracle_lib.ppgo_canonical_to_dir(C.c_float(x), C.c_float(y), d)
        dd = np.array(d[:])
        assert abs(np.linalg.norm(dd) - 1) < 1e-6 and abs(dd[2] - (2 * x - 1)) < 1e-6  # GP:586-595
        xy = (C.c_float * 2)()
        oracle_lib.ppgo_dir_to_canonical(d, xy)
        assert abs(xy[0] - x) < 1e-6 and min(abs(xy[1] - y), 1 - abs(xy[1] - y)) < 2e-5 / max(1e-3, np.sqrt(1 - dd[2] ** 2))
    bad = (C.c_float * 3)(float("nan"), 0, 0)
    xy = (C.c_float * 2)()
    oracle_lib.ppgo_dir_to_canonical(bad, xy)
    assert (xy[0], xy[1]) == (0.0, 0.0)  # GP:598-600
    ref = R.second_opinion()  # against the reference's canonicalToDir (libm sincos) and dirToCanonical (libm atan2)
    if ref is not None:
        pts = rng.rand(20000, 2).astype(np.float32)
        pts[:6] = [[0, 0], [1, 1], [0.5, 0.5], [1, 0], [0, 1], [0.25, 0.75]]
        ours = np.zeros((len(pts), 3), np.float32)
        for i, (x, y) in enumerate(pts):
            oracle_lib.ppgo_canonical_to_dir(C.c_float(x), C.c_float(y), d)
            ours[i] = d[:]
        theirs = ref.canonical_to_dir(pts)
        assert np.abs(ours.astype(np.float64) - theirs).max() <= R.SINCOS_TOL
        back = np.zeros((len(pts), 2), np.float32)
        for i in range(len(pts)):
            oracle_lib.ppgo_dir_to_canonical((C.c_float * 3)(*theirs[i]), xy)
            back[i] = xy[:]
        want = ref.dir_to_canonical(theirs)
        dy = np.abs(back[:, 1].astype(np.float64) - want[:, 1])
        dy = np.minimum(dy, 1 - dy)  # phi = 2 pi is phi = 0
        # x has no transcendental in it: exact.  y: the 4e-7 atan2 bound of test_detmath.py / 2 pi, plus an ulp at 1 for the two roundings of phi / (2 pi)
        assert np.array_equal(back[:, 0], want[:, 0]) and dy.max() <= 4e-7 / (2 * np.pi) + 2.0 ** -23


def _exercise(lib, acc, dfilter, xy, irr, w, q, seed=5, rho=0.01):
    n, m = len(irr), len(q)
    fp = C.POINTER(C.c_float)
    xy = np.ascontiguousarray(xy, np.float32); irr = np.ascontiguousarray(irr, np.float32)
    w = np.ascontiguousarray(w, np.float32); q = np.ascontiguousarray(q, np.float32)
    pdf = np.zeros(m, np.float32); smp = np.zeros((m, 2), np.float32)
    nn = C.c_uint32(); sums = np.zeros((65536, 4), np.float32); ch = np.zeros((65536, 4), np.uint16)
    sw, ts = C.c_float(), C.c_float()
    rc = lib.ppgo_dtree_exercise(acc, dfilter, C.c_float(rho), n, xy.ctypes.data_as(fp), irr.ctypes.data_as(fp), w.ctypes.data_as(fp), m,
                                 q.ctypes.data_as(fp), C.c_uint64(seed), pdf.ctypes.data_as(fp), smp.ctypes.data_as(fp), C.byref(nn),
                                 sums.ctypes.data_as(fp), ch.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(sw), C.byref(ts))
    assert rc == 0
    return dict(pdf=pdf, samples=smp, n=nn.value, sums=sums[:nn.value], children=ch[:nn.value], statw=sw.value, total=ts.value)


def test_dtree_pdf_integrates_to_one_and_matches_samples(oracle_lib):
    rng = np.random.RandomState(11)
    # a peaked distribution: most energy near (0.7, 0.2)
    xy = np.clip(np.concatenate([rng.normal([0.7, 0.2], 0.03, (6000, 2)), rng.rand(2000, 2)]), 0, 0.999999)
    irr = rng.uniform(0.5, 1.5, len(xy)); w = np.ones(len(xy))
    g = (np.stack(np.meshgrid(np.arange(256), np.arange(256)), -1).reshape(-1, 2) + 0.5) / 256
    for acc in (0, 1):  # fixed point and the reference's float accumulation agree to rounding
        r = _exercise(oracle_lib, acc, 0, xy, irr, w, g)
        assert 40 <= r["n"] <= 400 and r["statw"] == len(xy)
        assert abs(r["pdf"].mean() * 4 * np.pi - 1.0) < 1e-3  # pdf over the sphere integrates to 1 (GP:232-245, 420)
        s = r["samples"]
        frac_in_peak = ((np.abs(s[:, 0] - 0.7) < 0.1) & (np.abs(s[:, 1] - 0.2) < 0.1)).mean()
        assert frac_in_peak > 0.6  # samples follow the recorded energy (GP:257-301)
        # interior sums equal the sum of their children (build, GP:346-366)
        for k in range(r["n"]):
            for j in range(4):
                c = r["children"][k, j]
                if c:
                    assert abs(r["sums"][k, j] - r["sums"][c].sum()) <= 1e-5 * max(1.0, r["sums"][k, j])
    a, b = _exercise(oracle_lib, 0, 0, xy, irr, w, g), _exercise(oracle_lib, 1, 0, xy, irr, w, g)
    assert a["n"] == b["n"] and np.array_equal(a["children"], b["children"])  # same topology either way
    assert np.allclose(a["sums"], b["sums"], rtol=2e-4, atol=1e-4)


def test_dtree_box_filter_conserves_interior_energy(oracle_lib):
    rng = np.random.RandomState(2)
    xy = rng.uniform(0.3, 0.7, (3000, 2))  # far from the border: the box splat loses nothing (GP:403-409)
    irr = rng.uniform(0.5, 1.5, len(xy)); w = np.ones(len(xy))
    q = rng.rand(10, 2)
    near, box = _exercise(oracle_lib, 0, 0, xy, irr, w, q), _exercise(oracle_lib, 0, 1, xy, irr, w, q)
    assert abs(box["total"] - near["total"]) < 2e-3 * near["total"]
    # Near the border the part of the footprint outside [0,1]^2 is dropped (GP:403-409: a square of side 0.5^depthAt(p) centred on p,
    # density irradiance / side^2, recorded into the tree from its origin p - side / 2).  The exact loss follows from the depth of the
    # leaf quadrant that holds p, read off the returned topology: kept = (clipped side / side)^2 per axis.
    def depth_at(children, x, y):
        node, d = 0, 0
        while True:
            d += 1
            i = (1 if x >= 0.5 else 0) | (2 if y >= 0.5 else 0)
            x, y = (x * 2 if x < 0.5 else (x - 0.5) * 2), (y * 2 if y < 0.5 else (y - 0.5) * 2)
            if children[node, i] == 0:
                return d
            node = children[node, i]
    for px, py in ((0.001, 0.001), (0.0005, 0.4), (0.9995, 0.9999), (0.01, 0.01)):
        for acc in (0, 1):
            edge = _exercise(oracle_lib, acc, 1, np.tile(np.float32([px, py]), (100, 1)), np.ones(100), np.ones(100), q)
            side = 0.5 ** depth_at(edge["children"], np.float32(px), np.float32(py))
            kept = 1.0
            for c in (np.float32(px), np.float32(py)):
                kept *= (min(float(c) + side / 2, 1.0) - max(float(c) - side / 2, 0.0)) / side
            assert edge["statw"] == 100 and abs(edge["total"] - 100 * kept) < 2e-4 * 100, (px, py, acc, side, edge["total"], 100 * kept)
    assert abs(_exercise(oracle_lib, 0, 1, np.full((100, 2), 0.001), np.ones(100), np.ones(100), q)["total"] - 57.1536) < 1e-3   # side 1/256


def _floor_and_lamp(res, lamp_half=0.05, lamp_h=1.0):
    """A 20 x 20 diffuse floor (albedo 0.5) at y = 0 and a small square lamp (radiance 100) at height lamp_h
    facing down, seen from above by an orthogonal-ish narrow camera that does not see the lamp's front."""
    import ppg_host
    from ppg_host.scenes import SceneDesc
    P = np.array([[-10, 0, -10], [10, 0, -10], [10, 0, 10], [-10, 0, 10],
                  [-lamp_half, lamp_h, -lamp_half], [lamp_half, lamp_h, -lamp_half], [lamp_half, lamp_h, lamp_half], [-lamp_half, lamp_h, lamp_half]], np.float32)
    I = np.array([[0, 2, 1], [0, 3, 2],      # floor, normal +y
                  [4, 5, 6], [4, 6, 7]], np.uint32)  # lamp, normal -y
    cam = ppg_host.perspective_camera((0.0, 30.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 1), 4.0, "x", 0.1, 100.0, res, res)
    return SceneDesc(P, I, np.array([0, 0, 1, 1], np.uint32), np.array([-1, -1, 0, 0], np.int32),
                     [dict(type=0, reflectance=(0.5, 0.5, 0.5)), dict(type=0, reflectance=(0, 0, 0))],
                     [dict(radiance=(100.0, 100.0, 100.0))], cam)


def test_next_event_estimation_matches_the_analytic_direct_light(oracle_lib):
    """maxDepth = 2 (direct light only).  Under the lamp the floor's radiance is rho/pi * L * A * cos^2 / r^2 (small
    lamp: A = 0.01, r = 1).  nee = always (luminaire sampling + MIS, GP:1962-2021, 2083-2088) and nee = never must both
    converge to it; NEE with far less noise."""
    import ppg_host
    from conftest import make_oracle
    res = 24
    scene = _floor_and_lamp(res)
    # the camera sees a ~2.1 m wide patch centred under the lamp: analytic value per pixel
    half = 30.0 * np.tan(np.radians(2.0))
    xs = (np.arange(res) + 0.5) / res * 2 * half - half
    X, Z = np.meshgrid(xs, xs)
    r2 = X ** 2 + Z ** 2 + 1.0
    analytic = 0.5 / np.pi * 100.0 * 0.01 * (1.0 / r2) / r2  # cos = 1 / r at both ends
    out = {}
    for nee, budget in (("always", 64), ("never", 512)):
        e = make_oracle(oracle_lib, threads=16, budgetType="spp", budget=budget, maxDepth=2, rrDepth=10, nee=nee, seed=3)
        img = ppg_host.GuidedPathTracer(engine=e).render(scene)
        out[nee] = img[..., 0]
    assert abs(out["always"].mean() / analytic.mean() - 1) < 0.01
    assert abs(out["never"].mean() / analytic.mean() - 1) < 0.05
    err_nee = np.abs(out["always"] - analytic.T).mean() / analytic.mean()
    err_bsdf = np.abs(out["never"] - analytic.T).mean() / analytic.mean()
    assert err_nee < 0.03 and err_nee < err_bsdf / 4  # the profile matches pixel by pixel (the scene is symmetric, so .T is harmless)


def test_nee_modes_agree_on_cbox(oracle_lib):
    import ppg_host
    from conftest import CBOX_PROPS, make_oracle
    means = {}
    for nee in ("never", "always", "kickstart"):
        e = make_oracle(oracle_lib, threads=16, **dict(CBOX_PROPS, budget=31, nee=nee, seed=11))
        g = ppg_host.GuidedPathTracer(engine=e)
        means[nee] = g.render(ppg_host.cbox_scene(96, 96)).reshape(-1, 3).mean(0)
        if nee == "kickstart":  # both the path vertices and the direct-light vertices carry weight 0.5 (GP:2005, 2152)
            assert all(abs(it["tree"]["max_stat_weight"] * 2 - round(it["tree"]["max_stat_weight"] * 2)) < 1e-3 for it in g.iterations[1:2])
    for nee in ("always", "kickstart"):
        assert np.all(np.abs(means[nee] / means["never"] - 1) < 0.03), means


def test_light_through_a_thin_pane_matches_the_analytic_transmission(oracle_lib):
    """A thin-dielectric pane (eta 1.5) 20 cm above the floor: the lamp lights the floor, and the camera sees it, only through
    the pane's NULL component.  nee = never finds the lamp through the pane in rayIntersectAndLookForEmitter (GP:2184-2245);
    nee = always through Scene::evalTransmittance (scene.cpp:619-679); camera paths cross it by sampling the null lobe
    (GP:2045-2075).  All must give analytic direct light x T'(theta_light) x T'(theta_camera), T' = 1 - 2R / (1 + R) (slab with
    all internal reflections, thindielectric.cpp:160-164).  maxDepth = 5 gives the floor vertex (depth 2) an interaction budget
    maxDepth - depth - 1 = 2 and leaves none after a reflection off the pane, so only direct light arrives.
    (The pane is kept far from the lamp: with next-event estimation the reference computes the emitter pdf of a lamp found
    through a null surface from the distance to the LAST ray origin — records.inl:170-178 after GP:2218 — which skews the MIS
    weights when a null surface is close to the emitter.  The oracle reproduces that; this test stays clear of it.)"""
    import ppg_host
    from conftest import make_oracle
    res = 24
    scene = _floor_and_lamp(res)
    h, py = 1.7, 0.2
    pane = np.array([[-h, py, -h], [h, py, -h], [h, py, h], [-h, py, h]], np.float32)
    scene.positions = np.vstack([scene.positions, pane]).astype(np.float32)
    scene.indices = np.vstack([scene.indices, [[8, 9, 10], [8, 10, 11]]]).astype(np.uint32)
    scene.materials = list(scene.materials) + [dict(type="thindielectric", eta=1.5, reflectance=(1, 1, 1), specular=(1, 1, 1))]
    scene.tri_material = np.concatenate([scene.tri_material, [2, 2]]).astype(np.uint32)
    scene.tri_emitter = np.concatenate([scene.tri_emitter, [-1, -1]]).astype(np.int32)
    half = 30.0 * np.tan(np.radians(2.0))
    xs = (np.arange(res) + 0.5) / res * 2 * half - half
    X, Z = np.meshgrid(xs, xs)
    r2 = X ** 2 + Z ** 2 + 1.0

    def Tp(ci):
        ct = np.sqrt(1 - (1 - ci ** 2) / 1.5 ** 2)
        R = 0.5 * (((ci - 1.5 * ct) / (ci + 1.5 * ct)) ** 2 + ((1.5 * ci - ct) / (1.5 * ci + ct)) ** 2)
        return 1 - 2 * R / (1 + R)
    cam_cos = 30.0 / np.sqrt(X ** 2 + Z ** 2 + 30.0 ** 2)
    analytic = 0.5 / np.pi * 100.0 * 0.01 * (1.0 / r2) / r2 * Tp(1 / np.sqrt(r2)) * Tp(cam_cos)
    outside = (np.abs(X) > 0.15) | (np.abs(Z) > 0.15)  # the lamp's back hides the centre
    for nee, budget, tol in (("always", 64, 0.02), ("never", 4096, 0.06)):  # BSDF sampling of a 10 cm lamp: ~2 % noise at 4096 spp
        e = make_oracle(oracle_lib, threads=16, budgetType="spp", budget=budget, maxDepth=5, rrDepth=10, nee=nee, seed=4)
        img = ppg_host.GuidedPathTracer(engine=e).render(scene)[..., 0]
        assert abs(img[outside].mean() / analytic[outside].mean() - 1) < tol, (nee, img[outside].mean(), analytic[outside].mean())
    # without interaction budget (maxDepth = 3 → maxInteractions = 0 at the floor) the pane counts as an occluder (GP:2196, scene.cpp:636)
    e = make_oracle(oracle_lib, threads=16, budgetType="spp", budget=16, maxDepth=3, rrDepth=10, nee="always", seed=4)
    assert ppg_host.GuidedPathTracer(engine=e).render(scene)[..., 0][outside].max() == 0


def test_constant_environment_emitter_furnace_and_mis(oracle_lib):
    """A diffuse floor (albedo 0.5) under a constant sky of radiance (1, 2, 3) (emitters/constant.cpp): with direct light only the floor's
    radiance is albedo x L — exactly, for BSDF sampling (every cosine-sampled ray escapes and sees the sky: GP:2236-2243), and
    with luminaire sampling (cosine-hemisphere sampling about dRec.refN, constant.cpp:176-214) MIS-combined with it (GP:2083-2088,
    constant.cpp:216-231).  A second emitter (the lamp) makes the emitter pmf non-trivial (scene.cpp:375-380)."""
    import ppg_host
    from conftest import make_oracle
    res = 16
    scene = _floor_and_lamp(res)
    scene.environment = (1.0, 2.0, 3.0)
    scene.emitters = [dict(radiance=(0.0, 0.0, 0.0))]  # lamp switched off: still sampled with probability 1/2, contributes nothing
    scene.positions = scene.positions.copy(); scene.positions[4:8, 0] += 200.0  # ... and moved aside so that it does not hide the sky
    half = 30.0 * np.tan(np.radians(2.0))
    xs = (np.arange(res) + 0.5) / res * 2 * half - half
    X, Z = np.meshgrid(xs, xs)
    lit = np.ones_like(X, bool)
    for nee, budget in (("never", 8), ("always", 256), ("kickstart", 256)):
        e = make_oracle(oracle_lib, threads=16, budgetType="spp", budget=budget, maxDepth=2, rrDepth=10, nee=nee, seed=2, hideEmitters=1)
        img = ppg_host.GuidedPathTracer(engine=e).render(scene)
        want = 0.5 * np.array([1.0, 2.0, 3.0])
        m = img[lit].mean(0)
        if nee == "never":
            assert np.abs(img[lit] / want - 1).max() < 1e-5   # zero-variance: every sample returns albedo x L
        else:
            assert np.abs(m / want - 1).max() < 0.03, (nee, m)
    # the sky is visible to camera rays unless hideEmitters is set (GP:1906-1907)
    cam_up = ppg_host.perspective_camera((0.0, 1.0, 0.0), (0.0, 30.0, 0.0), (0, 0, 1), 4.0, "x", 0.1, 100.0, res, res)
    scene.camera = cam_up
    scene.positions = scene.positions.copy(); scene.positions[4:8, 1] = -5.0  # move the lamp out of view
    for hide, want in ((0, (1.0, 2.0, 3.0)), (1, (0.0, 0.0, 0.0))):
        e = make_oracle(oracle_lib, threads=4, budgetType="spp", budget=4, maxDepth=3, nee="never", seed=2, hideEmitters=hide)
        img = ppg_host.GuidedPathTracer(engine=e).render(scene)
        assert np.allclose(img.reshape(-1, 3), want)


def test_analytic_sphere_lamp_and_sky_sphere(oracle_lib):
    """shapes/sphere.cpp as an area emitter.  (1) A sphere lamp (radius r, radiance L) at height 1 over a diffuse floor: the irradiance
    from a uniform sphere is exactly pi L (r / D)^2 cos(theta), so with direct light only the floor shows rho L r^2 cos / D^2 — for
    BSDF sampling (the double-precision ray test, sphere.cpp:164-189, and Sphere::pdfDirect in the MIS weight) and for luminaire
    sampling (the cone of Sphere::sampleDirect, sphere.cpp:291-334).  (2) The camera INSIDE an emitting sphere with flipped normals
    and the default diffuse(0.5) BSDF — the sky dome of the reference's SPACESHIP scene: a furnace, every pixel L / (1 - 0.5); with
    next-event estimation the inside branch of sampleDirect (uniform area sampling, sphere.cpp:335-349) takes part."""
    import ppg_host
    from conftest import make_oracle
    res = 24
    scene = _floor_and_lamp(res)
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[:2], scene.tri_material[:2], scene.tri_emitter[:2]  # floor only
    r = 0.1
    scene.spheres = [dict(center=(0.0, 1.0, 0.0), radius=r, material=1, emitter=0)]
    half = 30.0 * np.tan(np.radians(2.0))
    xs = (np.arange(res) + 0.5) / res * 2 * half - half
    X, Z = np.meshgrid(xs, xs)
    D2 = X ** 2 + Z ** 2 + 1.0
    analytic = 0.5 * 100.0 * r * r / D2 / np.sqrt(D2)
    outside = (np.abs(X) > 0.2) | (np.abs(Z) > 0.2)  # the lamp itself hides the centre
    for nee, budget, tol in (("always", 64, 0.01), ("never", 1024, 0.04)):
        e = make_oracle(oracle_lib, threads=16, budgetType="spp", budget=budget, maxDepth=2, rrDepth=10, nee=nee, seed=3)
        img = ppg_host.GuidedPathTracer(engine=e).render(scene)[..., 0]
        assert abs(img[outside].mean() / analytic[outside].mean() - 1) < tol, (nee, img[outside].mean(), analytic[outside].mean())
        if nee == "always":
            assert np.abs(img - analytic.T)[outside].mean() / analytic[outside].mean() < 0.03
            assert img[res // 2, res // 2] > 50.0     # the camera sees the lamp itself in the centre
    # (2) the sky dome: one far-away triangle (the C-ABI wants a mesh), the camera at the dome's centre
    sky = _floor_and_lamp(8)
    sky.indices, sky.tri_material, sky.tri_emitter = sky.indices[:1], sky.tri_material[:1], sky.tri_emitter[:1]
    sky.positions = (sky.positions * np.float32(1e-3)).astype(np.float32); sky.positions[:, 1] -= 50.0
    sky.materials = list(sky.materials) + [dict(type="diffuse", reflectance=(0.5, 0.5, 0.5))]
    sky.emitters = [dict(radiance=(1.0, 2.0, 3.0))]
    sky.spheres = [dict(center=(0.0, 30.0, 0.0), radius=100.0, material=2, emitter=0, flip_normals=True)]
    for nee in ("never", "always"):
        e = make_oracle(oracle_lib, threads=16, budgetType="spp", budget=60, maxDepth=-1, rrDepth=100, nee=nee, seed=5)
        img = ppg_host.GuidedPathTracer(engine=e).render(sky)
        assert np.allclose(img.reshape(-1, 3).mean(0), [2.0, 4.0, 6.0], rtol=0.02), (nee, img.reshape(-1, 3).mean(0))
