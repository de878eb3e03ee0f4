"""What tests/test_hetmedia.py (CPU) and tests/test_hetmedia_gpu.py share: a numpy restatement, generic in dtype, of the reference's
heterogeneous medium under Woodcock tracking and of its volume data sources, written from the reference's text; the volumes, media and
items of the item-by-item tests; the margins.  Not a test module.

Restated (mitsuba/src/volume/constvolume.cpp, gridvolume.cpp, mitsuba/include/mitsuba/core/aabb.h, mitsuba/src/medium/heterogeneous.cpp):
  derive_volume(volume)      worldToGrid = scale((res - 1) / extents) * translate(-min) * toWorld^-1 and the world box of the eight
                             transformed corners (gridvolume.cpp:188-201), as the library's build stage derives them (double, rounded once)
  derive_medium(medium)      maxDensity = scale * (1 for a grid, the value for a const volume) and its inverse (heterogeneous.cpp:239-242);
                             the density's box: the world box of a grid, AABB's default (+inf, -inf) for a const volume
  lookup(V, p)               lookupFloat / lookupSpectrum: floorToInt, 0 where x1 < 0 .. z2 >= res, the trilinear expression in the
                             reference's order (gridvolume.cpp:337-388 and its RGB twin); a const volume answers its value
  aabb_clip(mn, mx, o, d)    AABB::rayIntersect (aabb.h:317-347), `return false` for a zero direction component outside [min, max] included
  sample_distance(...)       HeterogeneousMedium::sampleDistance, Woodcock branch (:613-662), mint = 0
  eval_transmittance(...)    HeterogeneousMedium::evalTransmittance with a sampler (:553-585): two tracked runs
  rand(key, dim)             ppg_rand (include/ppg_rng.h), vectorised
Evaluated in float32 it follows the device code's order of operations with numpy's log in place of the project's deterministic one; in
float64 it is the reference that is not the project's float code.  Both start from the same float32 tables.

Margins.  The device is compared against float64 within 8 x the largest difference between the float32 and the float64 evaluation over
the SAME items (figures(), measured on the CPU, never from the kernel), per quantity: `lookup` (absolute: texels live in [0, 1]), `t`
(relative to max(|t|, 1)), `sigma_s` and `transmittance` (relative to max(|value|, 1)).  Measured here (python tests/hetmedium_ref.py):
  lookup 1.6e-07  t 1.8e-07  sigma_s 4.6e-07  transmittance 1.0e-06
with 0.73 % of the lookup items and 0.20 % of a medium's tracking items undecided.

Items float64 cannot decide are left out ("undecided"): those whose chain of decisions holds a comparison closer than the margin —
  * a grid coordinate within COORD_MARGIN of the grid's outer boundary (0 or res - 1), where the lookup jumps between a texel's value and
    0 (between two cells it is continuous, so floor landing on either side of an inner integer decides nothing) — unless the float32 and
    the float64 evaluation of the coordinate agree bit for bit: then the arithmetic was exact (a grid placed by a quarter turn and
    power-of-two scales, the nodes and faces of LOOKUP_GRID_EXACT) and no precision places the point elsewhere;
  * t within T_MARGIN (relative) of maxt where a loop tests t < maxt;
  * density * invMaxDensity within ACCEPT_MARGIN of the random number it is compared with;
  * the box test of the ray within T_MARGIN of deciding otherwise (nearT against farT).
The item sets keep the undecided share below the 1 % the tests allow: about 3 expected steps per segment (asserted in tests/test_hetmedia.py).
"""
import numpy as np

f32 = np.float32
M32 = np.uint64(0xffffffff)
STEP_CAP = 65536        # PPG_HETMEDIUM_STEP_CAP
COORD_MARGIN = 1e-4     # grid units; float32 places a coordinate of a few units within a few 1e-7 of float64's
T_MARGIN = 1e-5         # relative; a few accumulated float32 roundings of t are below 1e-6
ACCEPT_MARGIN = 1e-5    # absolute, on density / maxDensity in [0, 1]


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _hash32(x):
    x = x & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def rand(key, dim):
    """ppg_rand(key, dim) for arrays of keys and dimensions: float32"""
    key, dim = np.asarray(key, np.uint64), np.asarray(dim, np.uint64)
    r = _hash32(key ^ _hash32((dim * np.uint64(0x9e3779b1) + np.uint64(0x7f4a7c15)) & M32))
    return (((r >> np.uint64(9)) | np.uint64(0x3f800000)).astype(np.uint32).view(f32) - f32(1.0)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- the tables
def derive_volume(v, channels, dtype=np.float64):
    """A volume dict (ppg_host.bindings.Volume's keys) as the lookups read it: float32 tables, cast to `dtype`"""
    f = dtype
    if "value" in v:
        a = np.asarray(v["value"], f32).reshape(-1)
        a = np.repeat(a, 3) if a.size == 1 else a
        return dict(const=True, channels=channels, value=a.astype(f))
    data = np.ascontiguousarray(v["data"], f32)
    rz, ry, rx = data.shape[:3]
    res = (rx, ry, rz)
    lo, hi = np.asarray(v["min"], f32), np.asarray(v["max"], f32)
    tw = np.eye(4, dtype=f32) if v.get("to_world") is None else np.asarray(v["to_world"], f32).reshape(4, 4)
    m = [[float(x) for x in row] for row in tw]  # (doubles from here, as the build stage)
    c = [[m[a][j] for a in range(3)] for j in range(3)]
    det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) + c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0])
    w2g = np.zeros((3, 4), f32)
    for i in range(3):
        a, b = c[(i + 1) % 3], c[(i + 2) % 3]
        li = [(a[1] * b[2] - a[2] * b[1]) / det, (a[2] * b[0] - a[0] * b[2]) / det, (a[0] * b[1] - a[1] * b[0]) / det]
        tr = -(li[0] * m[0][3] + li[1] * m[1][3] + li[2] * m[2][3])
        sc = (res[i] - 1) / (float(hi[i]) - float(lo[i]))
        for j in range(3):
            w2g[i, j] = f32(sc * li[j])
        w2g[i, 3] = f32(sc * (tr - float(lo[i])))
    mn, mx = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
    for corner in range(8):
        p = [hi[0] if corner & 1 else lo[0], hi[1] if corner & 2 else lo[1], hi[2] if corner & 4 else lo[2]]
        for a in range(3):
            w = f32(f32(f32(tw[a, 0] * p[0]) + f32(tw[a, 1] * p[1])) + f32(tw[a, 2] * p[2])) + tw[a, 3]
            mn[a], mx[a] = min(mn[a], w), max(mx[a], w)
    return dict(const=False, channels=channels, res=res, w2g=w2g.astype(f), data=data.reshape(-1, channels).astype(f), box=(mn, mx))


def derive_medium(medium, dtype=np.float64):
    """A heterogeneous medium dict as the tracking routines read it"""
    f = dtype
    dens, alb = derive_volume(medium["density"], 1, f), derive_volume(medium["albedo"], 3, f)
    scale = f32(medium.get("scale", 1.0))
    max_density = f32(scale * (f32(dens["value"][0]) if dens["const"] else f32(1.0)))
    inv = f32(f32(1.0) / max_density)
    box = (np.full(3, np.inf, f32), np.full(3, -np.inf, f32)) if dens["const"] else dens["box"]
    return dict(density=dens, albedo=alb, scale=f(scale), inv_max_density=f(inv), max_density=f(max_density), mn=box[0].astype(f), mx=box[1].astype(f))


# ---------------------------------------------------------------------------------------------------------------- the lookups
def grid_coords(V, p):
    """m_worldToGrid.transformAffine(p): [n, 3] in the volume's dtype"""
    w = V["w2g"]
    p = np.asarray(p, w.dtype)
    return np.stack([((w[i, 0] * p[:, 0] + w[i, 1] * p[:, 1]) + w[i, 2] * p[:, 2]) + w[i, 3] for i in range(3)], -1)


def lookup(V, p):
    """([n, channels] values, [n] the smallest distance of a grid coordinate from the grid's outer boundary — inf for a const volume)"""
    n = len(p)
    if V["const"]:
        f = V["value"].dtype
        return np.tile(V["value"][:V["channels"]][None, :], (n, 1)).astype(f), np.full(n, np.inf)
    f = V["w2g"].dtype.type
    g = grid_coords(V, p)
    res = np.asarray(V["res"])
    with np.errstate(all="ignore"):
        fl = np.floor(g)
        inside = np.isfinite(g).all(1) & (fl >= 0).all(1) & (fl + 1 < res[None, :]).all(1)
        edge = np.minimum(np.abs(g), np.abs(g - (res[None, :] - 1))).min(1).astype(np.float64)
    i1 = np.where(inside[:, None], fl, 0).astype(np.int64)
    fr = np.where(inside[:, None], g - fl, 0).astype(f)
    fx, fy, fz = fr[:, 0:1], fr[:, 1:2], fr[:, 2:3]
    _fx, _fy, _fz = f(1) - fx, f(1) - fy, f(1) - fz
    rx, ry = res[0], res[1]
    x1, y1, z1 = i1[:, 0], i1[:, 1], i1[:, 2]
    x2, y2, z2 = np.where(inside, x1 + 1, 0), np.where(inside, y1 + 1, 0), np.where(inside, z1 + 1, 0)
    D = V["data"]
    at = lambda z, y, x: D[(z * ry + y) * rx + x]  # noqa: E731
    d000, d001, d010, d011 = at(z1, y1, x1), at(z1, y1, x2), at(z1, y2, x1), at(z1, y2, x2)
    d100, d101, d110, d111 = at(z2, y1, x1), at(z2, y1, x2), at(z2, y2, x1), at(z2, y2, x2)
    val = ((d000 * _fx + d001 * fx) * _fy + (d010 * _fx + d011 * fx) * fy) * _fz + ((d100 * _fx + d101 * fx) * _fy + (d110 * _fx + d111 * fx) * fy) * fz
    return np.where(inside[:, None], val, f(0)).astype(f), edge


def aabb_clip(mn, mx, o, d):
    """AABB::rayIntersect: (hit [n], nearT, farT, the closest the answer came to being the other one)"""
    f = mn.dtype.type
    n = len(o)
    near, far = np.full(n, -np.inf, f), np.full(n, np.inf, f)
    hit = np.ones(n, bool)
    slack = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for i in range(3):
            zero = d[:, i] == 0
            out = zero & ((o[:, i] < mn[i]) | (o[:, i] > mx[i]))
            rcp = f(1) / np.where(zero, f(1), d[:, i])
            t1, t2 = (mn[i] - o[:, i]) * rcp, (mx[i] - o[:, i]) * rcp
            lo, hi = np.where(t1 > t2, t2, t1), np.where(t1 > t2, t1, t2)
            nn = np.where(~zero & hit, np.where(lo < near, near, lo), near)  # std::max(t1, nearT)
            ff = np.where(~zero & hit, np.where(far < hi, far, hi), far)   # std::min(t2, farT)
            near, far = nn, ff
            miss = ~zero & hit & ~(near <= far)
            gap = np.abs(far.astype(np.float64) - near.astype(np.float64))
            gap = np.where(np.isfinite(gap), gap / np.maximum(1.0, np.abs(near.astype(np.float64))), np.inf)
            slack = np.where(~zero & hit, np.minimum(slack, gap), slack)
            hit = hit & ~out & ~miss
    return hit, near, far, slack


# ---------------------------------------------------------------------------------------------------------------- tracking
def _track(M, o, d, mint, maxt, key, dim, active, accept_ends):
    """One tracked run per active item from t = mint: returns (event [n] — a collision was accepted —, t, density at t, dim after the
    run, undecided, capped).  Inactive items draw nothing."""
    f = M["scale"].dtype.type
    n = len(o)
    t = np.array(mint, f, copy=True)
    dim = np.array(dim, np.uint64, copy=True)
    event = np.zeros(n, bool)
    dens_t = np.zeros(n, f)
    undecided = np.zeros(n, bool)
    run = np.array(active, bool, copy=True)
    steps = 0
    with np.errstate(all="ignore"):
        while run.any():
            if steps == STEP_CAP:
                break
            steps += 1
            idx = np.nonzero(run)[0]
            u = rand(key[idx], dim[idx]).astype(f)
            dim[idx] += np.uint64(1)
            tt = t[idx] - np.log(f(1) - u) * M["inv_max_density"]
            t[idx] = tt
            left = ~(tt < maxt[idx])
            mt = maxt[idx].astype(np.float64)
            close = np.isfinite(mt) & (np.abs(tt.astype(np.float64) - mt) <= T_MARGIN * np.maximum(1.0, np.abs(mt)))
            undecided[idx] |= close
            run[idx[left]] = False
            idx, tt = idx[~left], tt[~left]
            if idx.size == 0:
                continue
            p = o[idx] + d[idx] * tt[:, None]
            val, edge = lookup(M["density"], p)
            density = val[:, 0] * M["scale"]
            u2 = rand(key[idx], dim[idx]).astype(f)
            dim[idx] += np.uint64(1)
            x = density * M["inv_max_density"]
            undecided[idx] |= (edge <= COORD_MARGIN) | (np.abs(x.astype(np.float64) - u2.astype(np.float64)) <= ACCEPT_MARGIN)
            acc = x > u2
            event[idx[acc]] = True
            dens_t[idx[acc]] = density[acc]
            run[idx[acc]] = False
    return event, t, dens_t, dim, undecided, run  # (run: still going at the cap)


def sample_distance(M, o, d, maxt, key, dim):
    """HeterogeneousMedium::sampleDistance on the rays (o, d) over [0, maxt]: dict(success, t, sigma_s [n, 3], transmittance, draws, dim,
    undecided)"""
    f = M["scale"].dtype.type
    o, d, maxt = np.asarray(o, f), np.asarray(d, f), np.asarray(maxt, f)
    key, dim0 = np.asarray(key, np.uint64), np.asarray(dim, np.uint64)
    hit, near, far, slack = aabb_clip(M["mn"], M["mx"], o, d)
    mint = np.where(near < f(0), f(0), near)   # std::max(mint, ray.mint)
    mx = np.where(maxt < far, maxt, far)       # std::min(maxt, ray.maxt)
    event, t, dens, dim, undecided, capped = _track(M, o, d, mint, mx, key, dim0, hit, True)
    undecided |= hit & (slack <= T_MARGIN)
    p = o + d * np.where(event, t, f(0))[:, None]
    albedo, edge = lookup(M["albedo"], p)
    undecided |= event & (edge <= COORD_MARGIN)
    with np.errstate(all="ignore"):
        tr = np.where(dens != 0, f(1) / np.where(dens != 0, dens, f(1)), f(0))
    tr = np.where(np.isfinite(tr), tr, f(0))
    return dict(success=event.astype(np.int32), t=np.where(event, t, f(0)), sigma_s=np.where(event[:, None], albedo * dens[:, None], f(0)),
                transmittance=np.where(event, tr, np.where(capped, f(0), f(1))), draws=(dim - dim0).astype(np.uint32), dim=dim, undecided=undecided)


def eval_transmittance(M, o, d, maxt, key, dim):
    """HeterogeneousMedium::evalTransmittance with a sampler on the rays (o, d) over [0, maxt]: dict(value — one of 0, 0.5, 1 —, draws, undecided)"""
    f = M["scale"].dtype.type
    o, d, maxt = np.asarray(o, f), np.asarray(d, f), np.asarray(maxt, f)
    key, dim0 = np.asarray(key, np.uint64), np.asarray(dim, np.uint64)
    hit, near, far, slack = aabb_clip(M["mn"], M["mx"], o, d)
    mint = np.where(near < f(0), f(0), near)
    mx = np.where(maxt < far, maxt, far)
    result = np.zeros(len(o), f)
    undecided = hit & (slack <= T_MARGIN)
    dim = dim0
    for _ in range(2):
        event, t, dens, dim, und, capped = _track(M, o, d, mint, mx, key, dim, hit, False)
        result = result + np.where(hit & ~event & ~capped, f(1), f(0))
        undecided |= und
    return dict(value=np.where(hit, result / f(2), f(1)), draws=(dim - dim0).astype(np.uint32), undecided=undecided)


# ---------------------------------------------------------------------------------------------------------------- volumes, media, items
def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) * c + s * K + (1 - c) * np.outer(a, a)


def placement(R, scale, translate):
    m = np.eye(4)
    m[:3, :3] = np.asarray(R) * scale
    m[:3, 3] = translate
    return m.astype(f32)


def _texels(shape, seed):
    return np.random.RandomState(seed).uniform(0.05, 1.0, shape).astype(f32)


# a quarter turn about z, a scale of 2 and dyadic offsets: every grid coordinate of a node or of a dyadic point is exact in float32
EXACT_TO_WORLD = placement([[0, -1, 0], [1, 0, 0], [0, 0, 1]], 2.0, (0.5, -1.0, 0.25))
SKEW_TO_WORLD = placement(rotation((1.0, 2.0, 0.5), 33.0), 1.3, (0.3, -0.2, 0.7))
# 5 x 4 x 3 nodes, one channel, spacing 0.5: the data box is (res - 1) / 2 wide, so worldToGrid scales by exactly 2 / 2
LOOKUP_GRID_EXACT = dict(data=_texels((3, 4, 5), 11), min=(0.0, 0.0, 0.0), max=(2.0, 1.5, 1.0), to_world=EXACT_TO_WORLD)
LOOKUP_GRID_RGB = dict(data=_texels((2, 3, 3, 3), 12), min=(-1.0, -0.5, 0.0), max=(1.0, 1.0, 0.8), to_world=SKEW_TO_WORLD)


def ramp_grid(to_world=None):
    """5 x 4 x 3 nodes over [0, 1]^3, the density rising linearly with x from 0.2 to 0.8"""
    x = np.linspace(0.2, 0.8, 5, dtype=np.float64)
    return dict(data=np.broadcast_to(x[None, None, :], (3, 4, 5)).astype(f32).copy(), min=(0.0, 0.0, 0.0), max=(1.0, 1.0, 1.0), to_world=to_world)


def holes_grid():
    """2 x 2 x 2 nodes over [-1, 1]^3 with empty corners: cells whose density falls to 0"""
    data = np.array([[[1.0, 0.0], [0.0, 0.5]], [[0.0, 0.75], [0.25, 0.0]]], f32)
    return dict(data=data, min=(-1.0, -1.0, -1.0), max=(1.0, 1.0, 1.0), to_world=placement(rotation((0.3, 1.0, 0.2), 20.0), 1.0, (0.1, 0.0, -0.1)))


ALBEDO_RGB = dict(data=_texels((2, 2, 2, 3), 13), min=(-4.0, -4.0, -4.0), max=(4.0, 4.0, 4.0), to_world=None)
# about 3 expected steps per segment: majorant 1.5 (const), 3 (ramp, a box of diagonal 1.7), 2 (holes, a box of diagonal 3.5)
TRACK_MEDIA = [
    ("const", dict(type="heterogeneous", density=dict(value=0.75), albedo=dict(value=(0.9, 0.5, 0.2)), scale=2.0)),
    ("ramp", dict(type="heterogeneous", density=ramp_grid(placement(rotation((0.0, 0.0, 1.0), 25.0), 1.0, (0.0, 0.0, 0.0))), albedo=ALBEDO_RGB, scale=3.0, phase="hg", g=0.3)),
    ("holes", dict(type="heterogeneous", density=holes_grid(), albedo=dict(value=0.8), scale=2.0)),
]
N_TRACK = 1024  # items per medium
TRACK_ITEM_DTYPE = np.dtype([("medium", "<i4"), ("o", "<f4", 3), ("d", "<f4", 3), ("maxt", "<f4"), ("key", "<u4"), ("dim", "<u4")])
LOOKUP_ITEM_DTYPE = np.dtype([("volume", "<i4"), ("p", "<f4", 3)])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def track_items(k, medium, n=N_TRACK):
    """Rays for medium k: through the density's box, from inside it, missing it; maxt before, inside and beyond the box and infinite; and,
    against the const density's default box, rays with a zero direction component (which AABB::rayIntersect refuses)."""
    rs = np.random.RandomState(100 + k)
    it = np.zeros(n, TRACK_ITEM_DTYPE)
    it["medium"] = k
    it["key"] = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    it["dim"] = rs.randint(0, 4096, n).astype(np.uint32)
    M = derive_medium(medium, np.float64)
    const = M["density"]["const"]
    centre = np.zeros(3) if const else (M["mn"] + M["mx"]) / 2
    radius = 1.0 if const else float(np.linalg.norm(M["mx"] - M["mn"]) / 2)
    target = centre + rs.uniform(-0.35, 0.35, (n, 3)) * radius
    kind = np.arange(n) % 4
    start = np.where((kind == 1)[:, None], centre + rs.uniform(-0.3, 0.3, (n, 3)) * radius, centre + _unit(rs.normal(size=(n, 3))) * radius * 2.5)
    d = _unit(target - start)
    miss = kind == 2  # aimed past the box
    d = np.where(miss[:, None], _unit(np.cross(d, rs.normal(size=(n, 3))) + 0.2 * d), d)
    if const:
        zero = kind == 3  # a zero direction component: the default box answers false
        d[zero, rs.randint(0, 3, int(zero.sum()))] = 0.0
        d = _unit(d)
    it["o"], it["d"] = start.astype(f32), d.astype(f32)
    reach = np.linalg.norm(target - start, axis=1)
    which = (np.arange(n) // 4) % 4
    maxt = np.where(which == 0, reach * rs.uniform(0.05, 0.4, n), np.where(which == 1, reach * rs.uniform(0.8, 1.2, n), np.where(which == 2, reach * 6.0, np.inf)))
    it["maxt"] = maxt.astype(f32)
    return it


def evaluate_track(medium, it, dtype):
    M = derive_medium(medium, dtype)
    s = sample_distance(M, it["o"], it["d"], it["maxt"], it["key"], it["dim"])
    e = eval_transmittance(M, it["o"], it["d"], it["maxt"], it["key"], s["dim"])
    return dict(success=s["success"], t=s["t"], sigma_s=s["sigma_s"], transmittance=s["transmittance"], draws=s["draws"], eval_transmittance=e["value"],
                eval_draws=e["draws"], undecided=s["undecided"] | e["undecided"])


def lookup_items(n=4096):
    """(items, volumes): volume 0 = LOOKUP_GRID_EXACT, 1 = LOOKUP_GRID_RGB.  Random interior points, every node exactly, points on each of
    the six faces and just outside them, far outside."""
    rs = np.random.RandomState(7)
    vols = [LOOKUP_GRID_EXACT, LOOKUP_GRID_RGB]
    parts = []
    for k, v in enumerate(vols):
        rz, ry, rx = v["data"].shape[:3]
        lo, hi = np.asarray(v["min"], np.float64), np.asarray(v["max"], np.float64)
        tw = np.asarray(v["to_world"], np.float64)
        local = []
        zz, yy, xx = np.meshgrid(np.arange(rz), np.arange(ry), np.arange(rx), indexing="ij")
        nodes = np.stack([xx.ravel() / (rx - 1.0), yy.ravel() / (ry - 1.0), zz.ravel() / (rz - 1.0)], -1)
        local.append(nodes)
        for axis in range(3):
            for side in (0.0, 1.0):
                # (dyadic in-face coordinates: exact under EXACT_TO_WORLD): two points on the face, six just outside it
                q = rs.randint(1, 8, (8, 3)) / 8.0
                q[:2, axis] = side
                q[2:, axis] = side + (1e-3 if side else -1e-3) * rs.uniform(1.0, 50.0, 6)
                local.append(q)
        local.append(rs.uniform(-8.0, 9.0, (64, 3)))  # far outside (mostly)
        fixed = np.concatenate(local)
        inner = rs.uniform(0.002, 0.998, (n // 2 - len(fixed), 3))
        u = np.concatenate([fixed, inner])
        p = (lo + u * (hi - lo)) @ tw[:3, :3].T + tw[:3, 3]
        it = np.zeros(len(u), LOOKUP_ITEM_DTYPE)
        it["volume"], it["p"] = k, p.astype(f32)
        parts.append(it)
    return np.concatenate(parts), vols


def evaluate_lookup(it, vols, dtype):
    """([n, 3] values — one-channel volumes in column 0 —, undecided)"""
    out = np.zeros((len(it), 3), dtype)
    undecided = np.zeros(len(it), bool)
    for k, v in enumerate(vols):
        sel = it["volume"] == k
        ch = 1 if np.asarray(v["data"]).ndim == 3 else 3
        V = derive_volume(v, ch, dtype)
        val, edge = lookup(V, it["p"][sel])
        out[sel, :ch] = val
        # exact arithmetic decides in every precision alike
        g32, g64 = grid_coords(derive_volume(v, ch, np.float32), it["p"][sel]), grid_coords(derive_volume(v, ch, np.float64), it["p"][sel])
        exact = (g32.astype(np.float64) == g64).all(1)
        undecided[sel] = (edge <= COORD_MARGIN) & ~exact
    return out, undecided


QUANTITIES = ("lookup", "t", "sigma_s", "transmittance")


def deviation(q, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dlt = np.abs(got - want)
    if q != "lookup":
        dlt = dlt / np.maximum(np.abs(want), 1.0)
    return dlt.reshape(dlt.shape[0], -1).max(axis=1) if dlt.ndim > 1 else dlt


def figures():
    """{quantity: the largest float32 / float64 difference of the restatement over the items, the undecided ones left out}"""
    fig = {q: 0.0 for q in QUANTITIES}
    it, vols = lookup_items()
    v32, u32 = evaluate_lookup(it, vols, np.float32)
    v64, u64 = evaluate_lookup(it, vols, np.float64)
    fig["lookup"] = float(deviation("lookup", v32, v64)[~u64].max())
    for k, (_, medium) in enumerate(TRACK_MEDIA):
        it = track_items(k, medium)
        r32, r64 = evaluate_track(medium, it, np.float32), evaluate_track(medium, it, np.float64)
        keep = ~r64["undecided"] & (r32["draws"] == r64["draws"])
        for q in ("t", "sigma_s", "transmittance"):
            fig[q] = max(fig[q], float(deviation(q, r32[q], r64[q])[keep].max()))
    return fig


def undecided_shares():
    """(the share of undecided lookup items, the largest share of undecided tracking items among the media, the largest share of decided
    items on which the float32 restatement draws another count than float64 — it should be none)"""
    it, vols = lookup_items()
    _, u = evaluate_lookup(it, vols, np.float64)
    worst, differ = 0.0, 0.0
    for k, (_, medium) in enumerate(TRACK_MEDIA):
        items = track_items(k, medium)
        r32, r64 = evaluate_track(medium, items, np.float32), evaluate_track(medium, items, np.float64)
        worst = max(worst, float(r64["undecided"].mean()))
        differ = max(differ, float((~r64["undecided"] & ((r32["draws"] != r64["draws"]) | (r32["eval_draws"] != r64["eval_draws"]))).mean()))
    return float(u.mean()), worst, differ


# measured by figures() (python tests/hetmedium_ref.py), asserted in tests/test_hetmedia.py
FIGURES = {"lookup": 1.6e-07, "t": 1.8e-07, "sigma_s": 4.6e-07, "transmittance": 1e-06}
MARGIN = {q: 8.0 * v for q, v in FIGURES.items()}

if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "practical-path-guiding_amd"))
    print({q: float("%.2g" % v) for q, v in figures().items()})
    print("undecided: lookups %.4f, tracking %.4f; decided items with other draw counts in float32: %.4f" % undecided_shares())
