"""What tests/test_normalmap.py (CPU) and tests/test_normalmap_gpu.py share: the scenes, the rays and a numpy restatement of the shading frame
of a normal-mapped or bump-mapped triangle that can be evaluated in float32 and in float64.  Not a test module.

The restatement follows the plug-ins and the kernels operation for operation: the triangle test of tests/traversal_ref.py (TriAccel), the
intersection record of csrc/ppg_device.h fill_isect_tex (its.uv, the UV tangents of TriMesh::computeUVTangents, the unperturbed shading
frame), BitmapTexture::eval / evalGradient on level 0 (mipmap.h:503-626), then NormalMap::getFrame (normalmap.cpp:108-124) or
BumpMap::getFrame (bumpmap.cpp:135-160).  In float64 — on the float32 inputs — it is the reference the test hook ppg_debug_shading_frame is
held to; in float32 it is what measures the tolerance (FRAME_FIGURE below).

Rays no float32 code can be held to are left out (`keep`): a hit within MARGIN of a triangle edge (the two evaluations may take different
triangles), a lookup within MARGIN of a texel border under `nearest`, and — for the bump map, whose gradient is constant per cell of the
bilinear lookup — a lookup within MARGIN of a cell border.  At most MAX_EXCLUDED of the rays of a case may be left out.
"""
import numpy as np

from traversal_ref import closest, tri_tuv, triaccel

f32, f64 = np.float32, np.float64
MARGIN = 1e-4
MAX_EXCLUDED = 0.01
N_RAYS = 1000  # per case; four cases
SEED = 20
# The largest deviation of the float32 restatement from the float64 one over the kept rays of all cases (the frame's components s, t, n,
# absolute; they are unit vectors), measured by tests/test_normalmap.py, which fails when it is exceeded — the two plug-ins separately:
FRAME_FIGURE = {"normal_map": 2.62e-6, "bump": 2.74e-6}  # measured 2.6147e-06 and 2.7385e-06; 4 x: 1.05e-5 and 1.10e-5
ALLOWANCE = 4  # the hook may differ from float64 by 4 x the figure: a different but legal contraction or ordering of the dot products


# ---------------------------------------------------------------------------------------------------------------- the scene
def normal_texels():
    """a 4 x 3 map of unit normals tilted up to 60 degrees from +z, one of them below the horizon (n.z < 0), as texels (n + 1) / 2"""
    rng = np.random.RandomState(7)
    tilt = np.radians(rng.uniform(5.0, 60.0, (3, 4)))
    phi = rng.uniform(0.0, 2 * np.pi, (3, 4))
    n = np.stack([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)], -1)
    below = np.array([0.55, 0.35, -0.3])
    n[1, 2] = below / np.linalg.norm(below)
    return ((n + 1.0) / 2.0).astype(f32)


def height_texels():
    """a 4 x 3 displacement map (monochrome) with slopes of the order of the quads' size"""
    rng = np.random.RandomState(11)
    return np.repeat((0.6 * rng.rand(3, 4, 1)).astype(f32), 3, 2)


# (filter, wrap u / v, uv scale, uv offset): the lookups leave [0, 1] in every case but the first
CASES = {
    "bilinear-repeat": dict(nearest=False, wrap_u="repeat", wrap_v="repeat", uv_scale=(1.0, 1.0), uv_offset=(0.0, 0.0)),
    "bilinear-clamp": dict(nearest=False, wrap_u="clamp", wrap_v="clamp", uv_scale=(1.9, -1.4), uv_offset=(-0.45, 1.2)),
    "nearest-repeat": dict(nearest=True, wrap_u="repeat", wrap_v="repeat", uv_scale=(2.6, 1.7), uv_offset=(-0.8, 0.35)),
    "nearest-clamp": dict(nearest=True, wrap_u="clamp", wrap_v="repeat", uv_scale=(1.3, 2.2), uv_offset=(-0.2, -0.6)),
}


def geometry():
    """Three quads of two triangles each in the plane z = 0, seen from +z: the first with texture coordinates (`vt`), the second without
    (NaN rows: its.uv is the barycentrics and dpdu the first edge), the third with texture coordinates and tilted vertex normals.  The
    scene has one normal array: the first two quads carry their face normal.  Every triangle has a material of its own, which names it."""
    pos, nrm, uv, idx = [], [], [], []
    rng = np.random.RandomState(3)
    for q, x0 in enumerate((-1.6, -0.5, 0.6)):
        corners = np.array([[x0, -0.5, 0.0], [x0 + 1.0, -0.45, 0.0], [x0 + 0.95, 0.5, 0.0], [x0 + 0.05, 0.55, 0.0]])
        base = len(pos)
        for k, c in enumerate(corners):
            pos.append(c)
            if q == 2:
                n = np.array([0.0, 0.0, 1.0]) + 0.35 * rng.uniform(-1, 1, 3) * np.array([1, 1, 0])
                nrm.append(n / np.linalg.norm(n))
            else:
                nrm.append([0.0, 0.0, 1.0])
            if q == 1:
                uv.append([np.nan, np.nan])
            else:  # a sheared, rotated parameterisation: dpdu is neither an edge nor an axis
                uv.append([0.9 * c[0] + 0.3 * c[1] + 0.2 * q, -0.25 * c[0] + 1.1 * c[1] + 0.4])
        idx += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return np.array(pos, f32), np.array(nrm, f32), np.array(uv, f32), np.array(idx, np.uint32)


def scene(case, key="normal_map", texels=None, res=(16, 12)):
    """the three quads with the adapter `key` ("normal_map" or "bump") around a diffuse BSDF, its texture looked up as CASES[case] says"""
    import ppg_host
    pos, nrm, uv, idx = geometry()
    if texels is None:
        texels = normal_texels() if key == "normal_map" else height_texels()
    mats = [dict({"type": 0, "reflectance": (0.5, 0.5, 0.5), key: 0}) for _ in range(len(idx))]
    cam = ppg_host.scenes.perspective_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, "x", 0.01, 100.0, *res)
    return ppg_host.SceneDesc(pos, idx, np.arange(len(idx), dtype=np.uint32), np.full(len(idx), -1, np.int32), mats, [], cam, normals=nrm,
                              environment=(1.0, 1.0, 1.0), texcoords=uv, textures=[dict(CASES[case], rgb=texels)])


def rays(case):
    """N_RAYS rays from above onto random points of the quads (a few miss), (o, mint, d, maxt) in float32"""
    rng = np.random.RandomState(SEED + list(CASES).index(case))
    target = np.stack([rng.uniform(-1.65, 1.65, N_RAYS), rng.uniform(-0.55, 0.6, N_RAYS), np.zeros(N_RAYS)], 1)
    origin = np.stack([rng.uniform(-2, 2, N_RAYS), rng.uniform(-2, 2, N_RAYS), rng.uniform(1.0, 4.0, N_RAYS)], 1)
    d = target - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((N_RAYS, 8), f32)
    out[:, 0:3], out[:, 4:7], out[:, 3], out[:, 7] = origin, d, 0.0, np.inf
    return out


# ---------------------------------------------------------------------------------------------------------------- vector helpers
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize(v):
    """v / |v| as vector.h:535-542, 625-627 do it: times the reciprocal of the length"""
    one = v.dtype.type(1.0)
    return v * (one / np.sqrt(dot(v, v)))[..., None]


# ---------------------------------------------------------------------------------------------------------------- the texture
def _texel(tex, x, y, wrap_u, wrap_v):
    h, w, _ = tex.shape
    out = []
    for c, size, mode in ((x, w, wrap_u), (y, h, wrap_v)):
        assert mode in ("repeat", "clamp")
        out.append(np.mod(c, size) if mode == "repeat" else np.clip(c, 0, size - 1))
    return tex[out[1], out[0]]


def _lookup_coordinates(tex, t, u, v, dtype):
    su, sv = (dtype(f32(x)) for x in t["uv_scale"])
    ou, ov = (dtype(f32(x)) for x in t["uv_offset"])
    return u * su + ou, v * sv + ov


def tex_eval(tex, t, u, v, dtype):
    """BitmapTexture::eval(uv) on level 0 (csrc/ppg_device.h tex_eval) -> rgb, and the distance of the lookup from the nearest branch
    point of the filter (a texel border under `nearest`; none under the bilinear filter, which is continuous)"""
    T = tex.astype(dtype)
    h, w, _ = T.shape
    ux, uy = _lookup_coordinates(tex, t, u, v, dtype)
    if t["nearest"]:
        a, b = ux * dtype(w), uy * dtype(h)
        margin = np.minimum(np.abs(a - np.round(a)), np.abs(b - np.round(b)))
        return _texel(T, np.floor(a).astype(int), np.floor(b).astype(int), t["wrap_u"], t["wrap_v"]), margin
    uu, vv = ux * dtype(w) - dtype(0.5), uy * dtype(h) - dtype(0.5)
    x0, y0 = np.floor(uu).astype(int), np.floor(vv).astype(int)
    dx1, dy1 = uu - x0.astype(dtype), vv - y0.astype(dtype)
    dx2, dy2 = dtype(1.0) - dx1, dtype(1.0) - dy1
    tx = lambda i, j: _texel(T, x0 + i, y0 + j, t["wrap_u"], t["wrap_v"])  # noqa: E731
    rgb = (((tx(0, 0) * dx2[:, None]) * dy2[:, None] + (tx(0, 1) * dx2[:, None]) * dy1[:, None]) + (tx(1, 0) * dx1[:, None]) * dy2[:, None]) \
        + (tx(1, 1) * dx1[:, None]) * dy1[:, None]
    return rgb, np.full(u.shape, np.inf)


def tex_gradient_lum(tex, t, u, v, dtype):
    """Texture2D::evalGradient over MIPMap::evalGradientBilinear(0, uv), luminance (csrc/ppg_device.h tex_gradient_lum) -> d/du, d/dv and the
    distance of the lookup from the nearest cell border, where the gradient jumps"""
    T = tex.astype(dtype)
    h, w, _ = T.shape
    ux, uy = _lookup_coordinates(tex, t, u, v, dtype)
    if t["nearest"]:
        z = np.zeros(u.shape, dtype)
        return z, z.copy(), np.full(u.shape, np.inf)
    uu, vv = ux * dtype(w) - dtype(0.5), uy * dtype(h) - dtype(0.5)
    margin = np.minimum(np.abs(uu - np.round(uu)), np.abs(vv - np.round(vv)))
    x0, y0 = np.floor(uu).astype(int), np.floor(vv).astype(int)
    dx, dy = (uu - x0.astype(dtype))[:, None], (vv - y0.astype(dtype))[:, None]
    tx = lambda i, j: _texel(T, x0 + i, y0 + j, t["wrap_u"], t["wrap_v"])  # noqa: E731
    p00, p10, p01, p11 = tx(0, 0), tx(1, 0), tx(0, 1), tx(1, 1)
    tmp = (p01 + p10) - p11
    one = dtype(1.0)
    g0 = ((p10 + p00 * (dy - one)) - tmp * dy) * dtype(w)
    g1 = ((p01 + p00 * (dx - one)) - tmp * dx) * dtype(h)
    g0 = g0 * dtype(f32(t["uv_scale"][0]))
    g1 = g1 * dtype(f32(t["uv_scale"][1]))
    lum = lambda g: (g[:, 0] * dtype(f32(0.212671)) + g[:, 1] * dtype(f32(0.715160))) + g[:, 2] * dtype(f32(0.072169))  # noqa: E731
    return lum(g0), lum(g1), margin


# ---------------------------------------------------------------------------------------------------------------- the frames
def frames(desc, ray_set, dtype):
    """Per ray, in `dtype`: the triangle hit (-1: none) — the index of its material, too —, its.uv, the unperturbed n and s, the frame
    (ps, pt, pn) the adapter hands the nested BSDF, and `keep`: the ray is far enough from every branch point to be compared."""
    pos, idx = np.asarray(desc.positions, f32), np.asarray(desc.indices)
    nrm, uvs = np.asarray(desc.normals, f32), np.asarray(desc.texcoords, f32)
    m = desc.materials[0]
    key = "normal_map" if m.get("normal_map") is not None else "bump"
    t = desc.textures[m[key]]
    tex = np.asarray(t["rgb"], f32)
    one = dtype(1.0)
    tt, uu, vv = tri_tuv(triaccel(pos, idx, dtype), ray_set, dtype)
    _, tri = closest(tt, uu, vv, ray_set, dtype)
    hit = tri >= 0
    r = np.arange(len(tri))
    k = np.where(hit, tri, 0)
    hu, hv = uu[r, k], vv[r, k]
    b = np.stack([one - hu - hv, hu, hv], 1)
    edge = np.min(b, axis=1)
    P = pos.astype(dtype)[idx[k]]
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    side1, side2 = p1 - p0, p2 - p0
    fn = cross(side1, side2)
    fn = fn * (one / np.sqrt(dot(fn, fn)))[:, None]
    N = nrm.astype(dtype)[idx[k]]
    shn = normalize((N[:, 0] * b[:, 0:1] + N[:, 1] * b[:, 1:2]) + N[:, 2] * b[:, 2:3])
    fn = np.where((dot(fn, shn) < 0)[:, None], -fn, fn)
    # its.uv and the UV tangents
    UV = uvs.astype(dtype)[idx[k]]
    has = ~np.isnan(UV[:, :, 0]).any(1)
    with np.errstate(invalid="ignore"):
        u = np.where(has, (UV[:, 0, 0] * b[:, 0] + UV[:, 1, 0] * b[:, 1]) + UV[:, 2, 0] * b[:, 2], b[:, 1])
        v = np.where(has, (UV[:, 0, 1] * b[:, 0] + UV[:, 1, 1] * b[:, 1]) + UV[:, 2, 1] * b[:, 2], b[:, 2])
        d1x, d1y = UV[:, 1, 0] - UV[:, 0, 0], UV[:, 1, 1] - UV[:, 0, 1]
        d2x, d2y = UV[:, 2, 0] - UV[:, 0, 0], UV[:, 2, 1] - UV[:, 0, 1]
        det = d1x * d2y - d1y * d2x
        assert np.all(det[has] != 0)
        inv = one / det
        dpdu = np.where(has[:, None], (side1 * d2y[:, None] - side2 * d1y[:, None]) * inv[:, None], side1)
        dpdv = np.where(has[:, None], (side1 * (-d2x)[:, None] + side2 * d1x[:, None]) * inv[:, None], side2)
    s = normalize(dpdu - shn * dot(shn, dpdu)[:, None])
    tv = cross(shn, s)
    if key == "normal_map":  # normalmap.cpp:108-124
        rgb, margin = tex_eval(tex, t, u, v, dtype)
        n = dtype(2.0) * rgb - one
        pn = normalize((s * n[:, 0:1] + tv * n[:, 1:2]) + shn * n[:, 2:3])
        ps = normalize(dpdu - pn * dot(pn, dpdu)[:, None])
        pt = cross(pn, ps)
    else:  # bumpmap.cpp:135-160
        gu, gv, margin = tex_gradient_lum(tex, t, u, v, dtype)
        du = dpdu + shn * (gu - dot(shn, dpdu))[:, None]
        dv = dpdv + shn * (gv - dot(shn, dpdv))[:, None]
        pn = normalize(cross(du, dv))
        ps = normalize(du - pn * dot(pn, du)[:, None])
        pt = cross(pn, ps)
        pn = np.where((dot(pn, fn) < 0)[:, None], -pn, pn)
    out = dict(uv=np.stack([u, v], 1), n=shn, s=s, ps=ps, pt=pt, pn=pn)
    assert all(x.dtype == dtype for x in out.values())
    out.update(tri=np.where(hit, tri, -1), keep=hit & (edge > MARGIN) & (margin > MARGIN), hit=hit)
    return out


def deviation(a, ref):
    """the largest absolute difference of the frames' components over the rays both keep and both attribute to the same triangle"""
    keep = ref["keep"] & (a["tri"] == ref["tri"])
    assert np.array_equal(a["tri"][ref["keep"]], ref["tri"][ref["keep"]])
    return max(float(np.abs(a[w][keep].astype(f64) - ref[w][keep]).max()) for w in ("ps", "pt", "pn"))


# ---------------------------------------------------------------------------------------------------------------- the null BSDF's depth count
def seen_through(k, max_depth):
    """GP:1917-1921, 2045-2075: whether a camera ray still reaches an emitter behind k null surfaces.  rRec.depth starts at 1; at every
    surface the loop stops when depth >= maxDepth (maxDepth != -1), and a sampled null interaction does rRec.depth++ and continues."""
    depth = 1
    for _ in range(k):
        if depth >= max_depth and max_depth != -1:
            return False
        depth += 1
    return True
