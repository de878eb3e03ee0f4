"""Scenes and batches of the emitter sampling tests (tests/test_emitter_sampling.py on the CPU, tests/test_emitter_sampling_gpu.py on the
device): a handful of triangles each, batches of 4096 to 16 384 items.  Everything is seeded; the same arrays go to the oracle, the device
and the restatement (tests/emitter_ref.py)."""
import ctypes as C
import math

import numpy as np

import ppg_host
from ppg_host.scenes import SceneDesc

import emitter_ref as ER

f32 = np.float32
TOP = 1.0 - 2.0 ** -23  # the largest value ppg_rand returns
MATS = [dict(type=0, reflectance=(0.5, 0.5, 0.5))]
MAP_SIZES = ((1, 1), (1, 2), (2, 1), (3, 5), (8, 16))


def sincos32(lib):
    """sin of include/ppg_detmath.h (ppg_sincos) through the oracle library's element-wise entry, for the envmap's float32 row weights"""
    def f(x):
        x = np.ascontiguousarray(x, f32)
        s, c, z = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
        fp = C.POINTER(C.c_float)
        assert lib.ppgo_math_eval(0, C.c_uint32(x.size), x.ctypes.data_as(fp), z.ctypes.data_as(fp), s.ctypes.data_as(fp), c.ctypes.data_as(fp)) == 0
        return s
    return f


def _camera():
    return ppg_host.perspective_camera((0.0, 0.5, 6.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, "x", 0.1, 100.0, 8, 8)


def _desc(P, I, tri_emitter, emitters, **kw):
    P, I = np.asarray(P, f32).reshape(-1, 3), np.asarray(I, np.uint32).reshape(-1, 3)
    return SceneDesc(P, I, np.zeros(len(I), np.uint32), np.asarray(tri_emitter, np.int32), list(MATS), emitters, _camera(), **kw)


# ------------------------------------------------------------------------------------------------------------------------------ scenes
LEGS = (1.0, 0.3, 0.03, 0.0, 0.01, 0.001)  # areas 0.5 .. 5e-7 (1 : 1e6) and a triangle of area 0 in the middle of the list


def mesh_scene(normals=False, shift=(0.0, 0.0, 0.0), legs=LEGS):
    """one emitter of 6 right triangles in the plane z = 0 facing +z, side by side along x; optionally vertex normals up to 60 degrees off"""
    P, I, x = [], [], -1.5
    for leg in legs:
        k = len(P)
        P += [(x, 0.0, 0.0), (x + leg, 0.0, 0.0), (x, leg, 0.0)] if leg else [(x, 0.0, 0.0), (x + 0.2, 0.0, 0.0), (x + 0.1, 0.0, 0.0)]
        I.append((k, k + 1, k + 2))
        x += max(leg, 0.2) + 0.05
    P = np.asarray(P, np.float64) + np.asarray(shift, np.float64)
    N = None
    if normals:
        rng = np.random.default_rng(5)
        tilt, az = np.radians(rng.uniform(0, 60, len(P))), rng.uniform(0, 2 * math.pi, len(P))
        N = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], 1).astype(f32)
    d = _desc(P, I, [0] * len(I), [dict(radiance=(3.0, 2.0, 1.0))], normals=N)
    d.camera = ppg_host.perspective_camera(tuple(np.asarray((0.0, 0.5, 6.0)) + shift), tuple(np.asarray(shift, np.float64)), (0, 1, 0), 40.0, "x", 0.1, 100.0, 8, 8)
    return d


def choice_scene(n, empty=None, env=False):
    """n area emitters of one small triangle each along x (emitter `empty` has none), optionally a constant environment as the last entry"""
    P, I, te = [], [], []
    for e in range(n):
        if e == empty:
            continue
        k = len(P)
        P += [(e - 0.2, -0.2, 0.0), (e + 0.2, -0.2, 0.0), (e, 0.3, 0.0)]
        I.append((k, k + 1, k + 2)); te.append(e)
    if not I:  # (a scene needs a triangle)
        P, I, te = [(9.0, 9.0, 9.0), (9.1, 9.0, 9.0), (9.0, 9.1, 9.0)], [(0, 1, 2)], [-1]
    return _desc(P, I, te, [dict(radiance=(1.0 + e, 2.0, 0.5)) for e in range(n)], environment=(0.5, 1.0, 2.0) if env else None)


def sphere_scene(flip=False):
    """an analytic sphere emitter of radius 0.5 at the origin and one small dark triangle far from everything the tests look at"""
    return _desc([(40.0, 40.0, 40.0), (40.1, 40.0, 40.0), (40.0, 40.1, 40.0)], [(0, 1, 2)], [-1], [dict(radiance=(2.0, 3.0, 4.0))],
                 spheres=[dict(center=(0.0, 0.0, 0.0), radius=0.5, material=0, emitter=0, flip_normals=bool(flip))])


SMALL_TRI = [(-0.1, -0.1, 0.0), (0.1, -0.1, 0.0), (0.0, 0.1, 0.0)]  # (a scene needs a triangle; it occludes few of the tests' rays)


def const_env_scene():
    return _desc(SMALL_TRI, [(0, 1, 2)], [-1], [], environment=(1.0, 2.0, 3.0))


def skew_rotation():
    """a rotation of 50 degrees about the axis (1, 2, 3), in float32"""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    t = math.radians(50.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K).astype(f32).reshape(-1)


def sun_map(h=32, w=64, seed=1):
    rng = np.random.RandomState(seed)
    rgb = (rng.rand(h, w, 3) ** 4).astype(f32) * 2
    rgb[6 * h // 32:9 * h // 32 + 1, 40 * w // 64:44 * w // 64 + 1] += 60.0
    return rgb


def random_map(h, w, seed=3):
    return (np.random.RandomState(seed + 7 * h + w).rand(h, w, 3) ** 3 * 4 + 0.01).astype(f32)


def black_variants():
    """8 x 16 maps with black parts: name -> rgb"""
    out = {}
    base = random_map(8, 16)
    for name, sl in (("first row", np.s_[0, :]), ("last row", np.s_[7, :]), ("first column", np.s_[:, 0]), ("last column", np.s_[:, 15])):
        m = base.copy(); m[sl] = 0; out[name] = m
    m = base.copy(); m[3, :] = 0; m[:, 6] = 0; out["interior row and column"] = m
    m = np.zeros_like(base); m[5, 11] = (7.0, 5.0, 3.0); out["one bright texel"] = m
    m = base.copy(); m[0, :] = 0; m[:, 0] = 0; out["first row and column"] = m
    return out


def envmap_scene(rgb, to_world=None, scale=1.5):
    return _desc(SMALL_TRI, [(0, 1, 2)], [-1], [],
                 envmap=dict(rgb=np.asarray(rgb, f32), scale=scale, to_world=np.eye(3, dtype=f32).reshape(-1) if to_world is None else to_world))


# ------------------------------------------------------------------------------------------------------------------------------ samples
def around(values):
    """every value, one ulp either side of it, 0 and the largest sample, clipped to [0, TOP]"""
    v = np.asarray(values, f32).reshape(-1)
    v = v[np.isfinite(v)]  # (the column cdf of a black row is 0 x inf)
    v = np.concatenate([v, np.nextafter(v, f32(2)), np.nextafter(v, f32(-1)), [f32(0), f32(TOP)]]).astype(f32)
    return np.unique(np.clip(v, f32(0), f32(TOP)))


def grid_with(edges_x, edges_y, n, rng):
    """n samples: the full grid of the edge values first (cropped to n), the rest uniform"""
    gx, gy = np.meshgrid(edges_x, edges_y, indexing="ij")
    u = np.stack([gx.ravel(), gy.ravel()], 1).astype(f32)
    if len(u) > n:
        u = u[rng.permutation(len(u))[:n]]
    rest = rng.uniform(0, 1, (n - len(u), 2)).astype(f32)
    return np.concatenate([u, np.minimum(rest, f32(TOP))]), len(u)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------------------ batches
N_BATCH = 4096


def choice_batches():
    """(name, desc, ref, ref_n, u): tables of 1, 2, 3 and 5 emitters, one without triangles as first, middle and last entry, with and
    without an environment emitter; u.x on every cdf entry, one ulp either side, 0 and the largest sample, then uniform"""
    out = []
    for n, empty, env in ((1, None, False), (2, None, True), (3, 0, False), (3, 1, True), (3, 2, False), (5, None, False), (5, 4, True), (5, 2, False)):
        desc = choice_scene(n, empty, env)
        cdf, _, _ = ER.f32_cdf([1.0] * (n + (1 if env else 0)))
        rng = np.random.default_rng(100 + 10 * n + (empty or 0))
        u, _ = grid_with(around(cdf), np.array([0.0, 0.25, 0.5, TOP], f32), N_BATCH, rng)
        ref = np.stack([rng.uniform(-1, n, N_BATCH), rng.uniform(-1, 1, N_BATCH), rng.uniform(0.5, 2, N_BATCH)], 1).astype(f32)
        ref_n = np.where(rng.uniform(size=(N_BATCH, 1)) < 0.5, [0.0, 0.0, -1.0], 0.0).astype(f32)
        out.append(("choice n=%d empty=%s env=%s" % (n, empty, env), desc, ref, ref_n, u))
    return out


def mesh_batch(normals, shift, n=N_BATCH, seed=21):
    """Reference points in a quarter each: in front with refN facing the emitter, in front with refN = 0, behind or with refN facing away,
    and within 1e-3 of the emitter's plane.  u.y on every area-cdf entry and one ulp either side; u.x at 0 and the largest sample, whose
    re-used value puts the point on a vertex; the rest uniform."""
    desc = mesh_scene(normals, shift)
    rng = np.random.default_rng(seed)
    R = ER.EmitterRef(desc)
    u, n_edge = grid_with(np.array([0.0, TOP, 0.5], f32), around(R.acdf[0]), n, rng)
    q = n // 4
    xy = rng.uniform(-2.0, 2.0, (n, 2))
    z = np.concatenate([rng.uniform(0.05, 3.0, 2 * q), rng.uniform(-3.0, 3.0, q), rng.uniform(-1e-3, 1e-3, n - 3 * q)])
    ref = (np.concatenate([xy, z[:, None]], 1) + np.asarray(shift, np.float64)).astype(f32)
    toward = unit(np.asarray(shift, np.float64) + (0.0, 0.3, 0.0) - ref + rng.normal(0, 0.3, (n, 3)))
    ref_n = toward.copy()
    ref_n[q:2 * q] = 0
    ref_n[2 * q:3 * q] = np.where((z[2 * q:3 * q] < 0)[:, None], toward[2 * q:3 * q], -toward[2 * q:3 * q])   # behind, or facing away
    ref_n[3 * q:] = np.where(rng.uniform(size=(n - 3 * q, 1)) < 0.5, 0.0, unit(rng.normal(size=(n - 3 * q, 3))))
    perm = rng.permutation(n)  # (every class of point meets the edge samples)
    return desc, ref[perm], ref_n.astype(f32)[perm], u, np.array(["front", "front no refN", "dark", "in plane"])[np.minimum(np.arange(n) // q, 3)][perm]


LEGS_EMPTY_FIRST = (0.0, 0.0, 1.0, 0.3, 0.0)  # two triangles of area 0 lead the list: only here does pmf_sample's forward skip decide


def leading_empty_batch(n=N_BATCH, seed=23):
    """The forward skip of DiscreteDistribution::sample matters for one input only: a sample of exactly 0 (lower_bound answers the first
    entry, whose interval is clamped to) in front of intervals of width 0.  u.y = 0 for a quarter of the items, an ulp and uniform else."""
    desc = mesh_scene(False, legs=LEGS_EMPTY_FIRST)
    rng = np.random.default_rng(seed)
    u = np.minimum(rng.uniform(0, 1, (n, 2)), TOP).astype(f32)
    u[:n // 4, 1] = 0
    u[n // 4:n // 4 + 64, 1] = np.nextafter(f32(0), f32(1))
    ref = (rng.uniform(-2.0, 2.0, (n, 3)) * (1, 1, 0) + (0, 0, 1) * rng.uniform(0.05, 3.0, (n, 1))).astype(f32)
    return desc, ref, np.zeros((n, 3), f32), u


def sphere_batch(flip, n=N_BATCH, seed=31):
    """Reference points at distances log-uniform from 0.55 to 5e3 radii, both sides of the switch at sinAlpha = 1 - 1e-4, inside, and at the
    centre exactly; refN zero for two thirds, random otherwise"""
    desc = sphere_scene(flip)
    rng = np.random.default_rng(seed)
    rad = 0.5
    q = n // 8
    r = rad * np.exp(rng.uniform(math.log(0.55), math.log(5e3), n))
    r[:q] = rad * rng.uniform(0.0, 1.0, q)                                     # inside
    r[q:2 * q] = rad / (1 - 1e-4) * (1 + rng.uniform(-3e-4, 3e-4, q))          # across the switch
    r[2 * q:2 * q + 16] = 0.0                                                  # the centre
    r[3 * q:3 * q + 128] = rad * np.exp(rng.uniform(math.log(5e3), math.log(2e4), 128))   # beyond: where 1 - sinAlpha^2 rounds to 1
    ref = (unit(rng.normal(size=(n, 3))) * r[:, None]).astype(f32)
    ref_n = np.where(rng.uniform(size=(n, 1)) < 2 / 3, 0.0, unit(rng.normal(size=(n, 3)))).astype(f32)
    u = np.minimum(rng.uniform(0, 1, (n, 2)), TOP).astype(f32)
    u[-64:, 0] = np.tile(np.array([0.0, TOP], f32), 32)
    return desc, ref, ref_n, u


def const_env_batch(n=N_BATCH, seed=41):
    """refN zero, on each side of the |x| > |y| switch of coordinateSystem, +-x, +-y, +-z exactly; reference points inside the bounding
    sphere, at its centre and outside it"""
    desc = const_env_scene()
    rng = np.random.default_rng(seed)
    R = ER.EmitterRef(desc)
    ref = (R.bs_c + unit(rng.normal(size=(n, 3))) * (R.bs_r * rng.uniform(0, 0.95, n) ** (1 / 3))[:, None]).astype(f32)
    ref[:256] = (R.bs_c + unit(rng.normal(size=(256, 3))) * R.bs_r * rng.uniform(1.05, 30, 256)[:, None]).astype(f32)   # outside
    ref[256:272] = R.bs_c.astype(f32)
    ref_n = unit(rng.normal(size=(n, 3)))
    k = n // 4
    ref_n[:k] = 0
    t = rng.uniform(-1, 1, k) * 1e-6   # |x| = |y| (1 + t): both sides of the switch
    ref_n[k:2 * k] = unit(np.stack([np.sign(rng.normal(size=k)) * (1 + t), np.sign(rng.normal(size=k)) * np.ones(k), rng.normal(size=k)], 1))
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    ref_n[2 * k:2 * k + 600] = np.tile(axes, (100, 1))
    u = np.minimum(rng.uniform(0, 1, (n, 2)), TOP).astype(f32)
    u[-64:] = np.array([[0, 0], [0.5, 0.5], [TOP, TOP], [0, TOP]], f32)[np.arange(64) % 4]
    return desc, ref, ref_n.astype(f32), u


def envmap_maps():
    """name -> (rgb, to_world)"""
    out = {}
    for h, w in MAP_SIZES:
        out["%dx%d" % (h, w)] = (random_map(h, w), None)
        out["%dx%d rotated" % (h, w)] = (random_map(h, w), skew_rotation())
    out["32x64 sun"] = (sun_map(), None)
    out["32x64 sun rotated"] = (sun_map(), skew_rotation())
    for name, m in black_variants().items():
        out["8x16 black " + name] = (m, None)
    return out


NAN_INPUTS = np.array([[0.0, 0.0], [0.0, 0.5], [0.5, 0.0]], f32)  # a sample component of exactly 0 in front of a black first row / column


def envmap_batch(rgb, to_world, lib, n=N_BATCH, seed=51):
    """Samples at 0, on every row and column cdf entry and one ulp either side, at the largest sample, and uniform — among the uniform ones
    the tent offset wraps posX below 0 and above w - 1 and pushes posY below 0 and above h - 1 by itself (asserted by the tests).  The
    first three items are NAN_INPUTS.  Reference points inside the bounding sphere, a few outside."""
    desc = envmap_scene(rgb, to_world)
    rng = np.random.default_rng(seed)
    R = ER.EmitterRef(desc, sincos32(lib))
    E = R.envmap
    ex = around(np.concatenate([E.cols[0], E.cols[E.h // 2], E.cols[E.h - 1]]))
    ey = around(E.rows)
    u, n_edge = grid_with(ex, ey, n // 2, rng)
    u = np.concatenate([NAN_INPUTS, u, np.minimum(rng.uniform(0, 1, (n - 3 - len(u), 2)), TOP).astype(f32)])
    ref = (R.bs_c + unit(rng.normal(size=(n, 3))) * (R.bs_r * rng.uniform(0, 0.9, n) ** (1 / 3))[:, None]).astype(f32)
    ref[-64:] = (R.bs_c + unit(rng.normal(size=(64, 3))) * R.bs_r * 3).astype(f32)
    ref_n = np.zeros((n, 3), f32)
    return desc, ref, ref_n, u, R


def envmap_directions(E, n=N_BATCH, seed=61):
    """Directions in the emitter's frame for eval and pdfDirection: a lat-long grid, +-y exactly, the seam (d.x = 0, d.z > 0, and one ulp
    either side in d.x), texel centre lines and one ulp either side"""
    rng = np.random.default_rng(seed)
    th = (np.arange(48) + 0.5) / 48 * math.pi
    ph = (np.arange(64) + 0.37) / 64 * 2 * math.pi
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    grid = np.stack([np.sin(TH) * np.sin(PH), np.cos(TH), -np.sin(TH) * np.cos(PH)], -1).reshape(-1, 3)
    poles = np.array([[0, 1, 0], [0, -1, 0], [1e-8, 1, 0], [0, -1, 1e-8]], np.float64)
    z = rng.uniform(0.05, 1, 64)
    seam = np.stack([np.zeros(64), rng.uniform(-0.9, 0.9, 64), z], 1)
    seam = np.concatenate([seam, seam + (1e-45, 0, 0), seam - (1e-45, 0, 0), seam + (1e-7, 0, 0), seam - (1e-7, 0, 0)])
    yy, xx = np.meshgrid(np.arange(E.h) + 0.5, np.arange(E.w) + 0.5, indexing="ij")   # texel centres: u = x + 0.5 - 0.5 lies on a texel line
    tc, pc = yy.ravel() / E.h * math.pi, xx.ravel() / E.w * 2 * math.pi
    centres = np.stack([np.sin(tc) * np.sin(pc), np.cos(tc), -np.sin(tc) * np.cos(pc)], 1)[:512]
    c32 = centres.astype(f32)
    centres = np.concatenate([c32, np.nextafter(c32, f32(2)), np.nextafter(c32, f32(-2))]).astype(np.float64)
    d = np.concatenate([grid, poles, seam, centres])
    return np.concatenate([d, unit(rng.normal(size=(max(0, n - len(d)), 3)))]).astype(f32)[:max(n, len(d))]


# ------------------------------------------------------------------------------------------------------------------------------ checks
FIELDS = ("d", "n", "dist", "pdf", "value", "sd", "sdist")


def bits_equal(a, b):
    """two structured arrays, every byte (NaN patterns included)"""
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(a, b):
    for name in a.dtype.names:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        bad = (x.view(np.uint32) != y.view(np.uint32)).reshape(len(a), -1).any(1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            return "%s differs in %d items, first %d: %s vs %s" % (name, bad.sum(), i, a[name][i], b[name][i])
    return "equal"


def check_against_restatement(name, got, R, cap_on=None, allow_inf_pdf=False):
    """The record `got` (oracle's or device's) against the restatement R: the discrete outputs exactly on every item; dark samples exactly 0;
    every continuous field within its bound on the items the restatement does not leave out and whose bound is below 1e-2 relative.
    Prints the counts per class and the largest error-to-bound ratio per field; asserts the 2 % cap on what is left out (over the items
    `cap_on`, default all).  -> the ratios"""
    n = len(got)
    known = R["kind"] != "other"
    assert (got["emitter"] == R["emitter"]).all(), name
    assert (got["em_pdf"] == R["em_pdf"]).all(), name
    assert (got["is_env"] == R["is_env"]).all() and (got["is_delta"][known] == 0).all(), name
    finite = np.isfinite(got["value"]).all(1) & np.isfinite(got["d"]).all(1) & np.isfinite(got["n"]).all(1) & np.isfinite(got["dist"]) & ~np.isnan(got["pdf"])
    centre = ~np.isfinite(R["d"]).all(1)  # (a reference point at a sphere's centre: refToCenter / 0 in the reference as well)
    assert finite[known & ~centre].all(), (name, np.flatnonzero(~finite & known & ~centre)[:8])
    if not allow_inf_pdf:
        assert np.isfinite(got["pdf"]).all(), name
    with np.errstate(all="ignore"):
        firm = ((R["kind"] != "sphere") | ((R["tol_n"] <= 1e-2) & (R["tol_d"] <= 1e-2))) & ~centre   # (emitter_ref.py: a sphere that subtends too little)
    ok = known & ~R["skip"] & firm
    lit_got = (got["value"] != 0).any(1)
    bad = ok & (lit_got != R["lit"])
    assert not bad.any(), (name, "lit / dark differs", np.flatnonzero(bad)[:8])
    dark = ok & ~R["lit"] & (R["pdf"] == 0)
    assert (got["pdf"][dark] == 0).all() and (got["value"][dark] == 0).all(), name
    ratios = {}
    counted = {}
    for k in FIELDS:
        a, b, tol = got[k].astype(np.float64), R[k], R["tol_" + k]
        with np.errstate(all="ignore"):
            size = np.abs(b).max(1) if b.ndim == 2 else np.abs(b)
            sel = ok & (R["sampled"] if k not in ("pdf", "value") else R["lit"] | (R["pdf"] != 0))
            if k in ("pdf", "value", "dist", "sdist"):
                sel = sel & ((R["kind"] != "sphere") | (tol <= 1e-2 * size))
            err = np.abs(a - b)
            err = err.max(1) if err.ndim == 2 else err
            ratio = np.where(sel, err / tol, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        ratios[k], counted[k] = float(ratio.max()) if n else 0.0, int(sel.sum())
    over = cap_on if cap_on is not None else np.ones(n, bool)
    left_out = int((R["skip"] & known & over).sum())
    classes = {c: int((R["kind"] == c).sum()) for c in np.unique(R["kind"])}
    print("%s: %d items %s; lit %d, dark %d, left out %d of %d, bound too loose %d; compared %s; largest error / bound %s" % (
        name, n, classes, int((ok & R["lit"]).sum()), int((ok & ~R["lit"]).sum()), left_out, int(over.sum()), int((known & ~R["skip"] & ~firm).sum()),
        counted, {k: round(v, 4) for k, v in ratios.items()}))
    assert left_out <= 0.02 * over.sum(), (name, left_out)
    for k, v in ratios.items():
        assert v <= 1.0, (name, k, v)
    return ratios
