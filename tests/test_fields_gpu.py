"""Feature buffers of the first hit on the GPU (include/ppg.h ppg_render_fields; csrc/ppg_fields_kernels.h): the camera rays against a numpy
restatement of k_generate's, the fields against the pinned ray hooks bit for bit, primIndex / relPosition / albedo against float64, the
filtered images against the documented summation order (j, dy, dx) in float32, determinism, and a render left untouched."""
import ctypes as C

import numpy as np
import pytest

from test_rfilter_gpu import FILTERS, _rand, np_splat
from test_textures import _np_lookup

f32 = np.float32
pytestmark = pytest.mark.gpu

SEED = 7
ALL = ["position", "relPosition", "distance", "geoNormal", "shNormal", "uv", "albedo", "primIndex"]
NAN = float("nan")
UNDEF = [(-1.0, -2.0, -3.0), NAN, -1.0, (0.0, 0.0, 0.0), (0.5, NAN, 0.25), (-7.0, -7.0, -7.0), 9.0, -1.0]  # one per field of ALL
UNDEF_FINITE = [(-1.0, -2.0, -3.0), 4.0, -1.0, (0.0, 0.0, 0.0), (0.5, 0.125, 0.25), (-7.0, -7.0, -7.0), 9.0, -1.0]


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**dict(dict(budgetType="spp", budget=8, sppPerPass=1, seed=SEED), **props))


# ---- the hand-made 17 x 13 scene: a 4 x 3 grid of patches in the plane z = 0 seen from z = 10; the view reaches past its edge ----
HW, HH = 17, 13
SLOT_X, SLOT_Y, HALF = (-3.3, -1.1, 1.1, 3.3), (-2.2, 0.0, 2.2), 0.9
QUAD_SLOTS = [0, 1, 5, 6, 7, 8, 9, 10]  # slot -> a quad of two triangles (2 q, 2 q + 1, q = its place in this list); its material = the slot
SPHERE_SLOT, DISK_SLOT, CYL_SLOT = 2, 3, 4  # slot 11 stays empty
UV_SLOTS = (0, 5, 6)  # quads with texture coordinates
TEX = np.random.RandomState(5).rand(8, 16, 3).astype(f32) * f32(0.8) + f32(0.1)
NMAP = (np.random.RandomState(6).rand(4, 4, 3) * [0.4, 0.4, 0.2] + [0.3, 0.3, 0.8]).astype(f32)
OPAC = (np.random.RandomState(7).rand(4, 8, 3) * 0.7 + 0.2).astype(f32)
MATERIALS = [
    dict(type="diffuse", reflectance=tuple(float(v) for v in TEX.reshape(-1, 3).mean(0)), texture=0),
    dict(type="diffuse", reflectance=(0.2, 0.4, 0.6)),
    dict(type="roughdiffuse", reflectance=(0.3, 0.5, 0.7), alpha=0.3),
    dict(type="phong", reflectance=(0.15, 0.25, 0.35), specular=(0.2, 0.2, 0.2), exponent=20.0),
    dict(type="diffuse", reflectance=(0.6, 0.3, 0.1), twosided=True),
    dict(type="diffuse", reflectance=(0.45, 0.55, 0.65), normal_map=1),
    dict(type="diffuse", reflectance=(0.7, 0.6, 0.5), opacity=(0.5, 0.5, 0.5), opacity_texture=2),
    dict(type="plastic", reflectance=(0.35, 0.15, 0.55), eta=1.49),
    dict(type="roughplastic", reflectance=(0.25, 0.65, 0.45), alpha=0.1, eta=1.49, rtrans=0),
    dict(type="conductor", eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2)),
    dict(type="diffuse", reflectance=(0.5, 0.2, 0.3), coating=dict(kind="coating", eta=1.5, thickness=1.0, sigma_a=0.1)),
]
CYL_R, CYL_LEN = 0.6, 1.6
CYL_ROT = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)  # object z (the axis) -> world x


def _slot_centre(s):
    return np.array([SLOT_X[s % 4], SLOT_Y[s // 4], 0.0])


def hand_scene(lens=None, rfilter=None, blend=False):
    import ppg_host
    pos, uv, idx = [], [], []
    for s in QUAD_SLOTS:
        c = _slot_centre(s)
        base = len(pos)
        for k, (dx, dy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):  # counter-clockwise from +z: the normal faces the camera
            pos.append(c + [dx * HALF, dy * HALF, 0.0])
            uv.append([(dx + 1) / 2, (dy + 1) / 2] if s in UV_SLOTS else [NAN, NAN])
        idx += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    tmat = np.repeat(np.array(QUAD_SLOTS, np.uint32), 2)
    materials = [dict(m) for m in MATERIALS]
    if blend:  # the plain diffuse quad becomes a blend of two diffuse children
        materials[1] = dict(type=0, blend=dict(kind="blendbsdf", weight=0.25, children=[dict(type="diffuse", reflectance=(0.2, 0.4, 0.6)),
                                                                                        dict(type="diffuse", reflectance=(0.6, 0.4, 0.2))]))
    cs, cd, cc = _slot_centre(SPHERE_SLOT), _slot_centre(DISK_SLOT), _slot_centre(CYL_SLOT)
    spheres = [dict(center=tuple(cs), radius=HALF, material=SPHERE_SLOT)]
    shapes = [dict(type="disk", to_world=np.hstack([np.eye(3) * HALF, cd[:, None]]), material=DISK_SLOT),
              dict(type="cylinder", to_world=np.hstack([CYL_ROT, (cc - [CYL_LEN / 2, 0, 0])[:, None]]), radius=CYL_R, length=CYL_LEN, material=CYL_SLOT)]
    cam = ppg_host.scenes.perspective_camera((0.3, -0.2, 10.0), (0.0, 0.0, 0.0), (0, 1, 0), 55.0, "x", 0.01, 100.0, HW, HH)
    tex = [dict(rgb=TEX), dict(rgb=NMAP, wrap_u="clamp", wrap_v="clamp"), dict(rgb=OPAC)]
    return ppg_host.SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), tmat, np.full(len(idx), -1, np.int32), materials, [], cam,
                              environment=(1.0, 1.0, 1.0), rtrans=np.full((1, 33), 0.9, f32), spheres=spheres, texcoords=np.array(uv, f32), textures=tex,
                              shapes=shapes, lens=lens, rfilter=rfilter)


LENS = dict(aperture_radius=0.35, focus_distance=10.0)


def _desc(name, rfilter=None):
    import ppg_host
    if name == "cbox":
        d = ppg_host.cbox_scene(67, 41)
    elif name == "room":
        d = ppg_host.room_scene(67, 41, n_boxes=40, tess=1)
    else:
        return hand_scene(lens=LENS if name == "lens" else None, rfilter=rfilter)
    d.rfilter = rfilter
    return d


_CACHE = {}


def samples(name, first=0):
    """per scene and sample index, computed once: the engine (box filter), the hook's camera rays with their intersection and frame
    records, and every field's value of that ONE sample per pixel (spp = 1, box filter: the image is the sample)"""
    key = (name, first)
    if key not in _CACHE:
        if ("engine", name) not in _CACHE:
            e = hip()
            e.set_scene(_desc(name))
            _CACHE[("engine", name)] = e
        e = _CACHE[("engine", name)]
        rays = e.debug_camera_rays(first, 1)[0]
        fields = e.render_fields(ALL, spp=1, undefined=UNDEF, first_sample=first)
        _CACHE[key] = dict(engine=e, rays=rays, hit=e.debug_intersect(rays), frame=e.debug_shading_frame(rays), fields=fields)
    return _CACHE[key]


def ulps(a, b):
    """distance in units in the last place of float32 values (of equal sign, or both zero)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


# ---- 1. rays ----
def _np_rays(cam, seed, sample, W, H):
    """camera_ray (csrc/ppg_device.h) of the pinhole in float32, operation by operation"""
    s2c, c2w = np.asarray(cam["sample_to_camera"], f32).reshape(4, 4), np.asarray(cam["camera_to_world"], f32).reshape(4, 4)
    pix = np.arange(W * H, dtype=np.uint32)
    sx = (pix % W).astype(f32) + _rand(seed, pix, sample, 0)
    sy = (pix // W).astype(f32) + _rand(seed, pix, sample, 1)
    inv_w, inv_h = f32(1) / f32(W), f32(1) / f32(H)
    px, py, pz = sx * inv_w, sy * inv_h, np.zeros_like(sx)
    row = lambda m: ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]  # noqa: E731
    x, y, z, w = row(s2c[0]), row(s2c[1]), row(s2c[2]), row(s2c[3])
    r = f32(1) / w
    near = np.stack([np.where(w == 1, x, x * r), np.where(w == 1, y, y * r), np.where(w == 1, z, z * r)])
    length = np.sqrt((near[0] * near[0] + near[1] * near[1]) + near[2] * near[2])
    dl = near * (f32(1) / length)
    inv_z = f32(1) / dl[2]
    d = np.stack([(c2w[i, 0] * dl[0] + c2w[i, 1] * dl[1]) + c2w[i, 2] * dl[2] for i in range(3)], 1)
    return c2w[:3, 3], d, f32(cam["near_clip"]) * inv_z, f32(cam["far_clip"]) * inv_z, (sx, sy)


@pytest.mark.parametrize("name", ["cbox", "hand"])
def test_camera_rays_are_k_generates(name):
    e = samples(name)["engine"]
    desc = _desc(name)
    W, H = desc.camera["width"], desc.camera["height"]
    got = e.debug_camera_rays(0, 6)
    assert got.shape == (6, W * H, 8) and np.array_equal(got[0], samples(name)["rays"])
    for j in (0, 1, 5):
        o, d, mint, maxt, _ = _np_rays(desc.camera, SEED, j, W, H)
        assert np.array_equal(got[j, :, 0:3], np.broadcast_to(o, (W * H, 3)))  # the pinhole: exactly the camera position
        assert ulps(got[j, :, 4:7], d).max() <= 4 and ulps(got[j, :, 3], mint).max() <= 4 and ulps(got[j, :, 7], maxt).max() <= 4
    assert not np.array_equal(got[0], got[1])


def test_lens_rays_start_on_the_aperture_and_cross_the_focus_plane():
    e = samples("lens")["engine"]
    desc = _desc("lens")
    cam = desc.camera
    c2w = np.asarray(cam["camera_to_world"], np.float64).reshape(4, 4)
    got = e.debug_camera_rays(0, 6).astype(np.float64)
    for j in (0, 1, 5):
        o_cam = (got[j, :, 0:3] - c2w[:3, 3]) @ c2w[:3, :3]  # (a rotation: its inverse is its transpose)
        # (float32 world coordinates of magnitude 10: 1e-5 covers their rounding)
        assert np.abs(o_cam[:, 2]).max() < 1e-5 and np.hypot(o_cam[:, 0], o_cam[:, 1]).max() <= LENS["aperture_radius"] + 1e-5
        assert np.unique(np.round(o_cam[:, :2], 6), axis=0).shape[0] > HW * HH // 2  # every path has its own origin
        # the pinhole ray of the same film position meets the lens ray on the focus plane
        _, d_pin, _, _, _ = _np_rays(cam, SEED, j, HW, HH)
        d_pin = d_pin.astype(np.float64) @ c2w[:3, :3]
        focus = d_pin * (LENS["focus_distance"] / d_pin[:, 2:3])
        d_cam = got[j, :, 4:7] @ c2w[:3, :3]
        t = (LENS["focus_distance"] - o_cam[:, 2]) / d_cam[:, 2]
        assert np.abs(o_cam + d_cam * t[:, None] - focus).max() < 1e-4
        assert np.abs(np.linalg.norm(got[j, :, 4:7], axis=1) - 1).max() < 1e-6


# ---- 2. the fields are the pinned hooks', bit for bit ----
def _same(a, b):
    """equal bit patterns up to the sign of zero and the payload of NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("name", ["cbox", "room", "hand", "lens"])
def test_fields_equal_the_hooks_bit_for_bit(name, first):
    s = samples(name, first)
    F, hit, frame = s["fields"], s["hit"], s["frame"]
    H, W = F["position"].shape[:2]
    flat = {k: v.reshape(H * W, 3) for k, v in F.items()}
    on = hit["prim"] >= 0
    assert on.any() and np.array_equal(frame["prim"], hit["prim"])
    if name in ("hand", "lens"):
        assert (~on).sum() > 10  # the view reaches past the geometry
    assert np.array_equal(flat["position"][on], hit["p"][on])
    assert np.array_equal(flat["distance"][on], np.repeat(hit["t"][on, None], 3, 1))
    assert np.array_equal(flat["geoNormal"][on], hit["geo_n"][on]) and np.array_equal(flat["shNormal"][on], hit["n"][on])
    for k, name_k in enumerate(ALL):
        want = np.broadcast_to(np.asarray(UNDEF[k], f32), (3,))
        assert _same(flat[name_k][~on], np.broadcast_to(want, ((~on).sum(), 3))), name_k
    assert np.isnan(flat["relPosition"][~on]).all() or not (~on).any()
    assert np.array_equal(flat["uv"][on][:, 2], np.zeros(on.sum(), f32))
    if name in ("hand", "lens"):
        prim = flat["primIndex"][:, 0].astype(np.int64)
        textured = on & np.isin(prim // 2, [QUAD_SLOTS.index(q) for q in UV_SLOTS]) & (prim < 2 * len(QUAD_SLOTS))
        assert textured.sum() > 5 and np.array_equal(flat["uv"][textured][:, :2], frame["uv"][textured])
        assert (np.abs(frame["uv"][textured]) > 0).any()
        analytic = on & (prim >= 2 * len(QUAD_SLOTS))
        assert analytic.sum() > 5 and not flat["uv"][analytic].any()
        # the quad without coordinates: the barycentrics (b1, b2) of the hit, from its position
        for tri in (2, 3):
            m = on & (prim == tri)
            c, h = _slot_centre(1), HALF
            corners = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]]) + c
            a, b_, c_ = corners[0], corners[tri - 1], corners[tri]
            p = flat["position"][m].astype(np.float64) - a
            sol = np.linalg.lstsq(np.stack([b_ - a, c_ - a], 1), p.T, rcond=None)[0].T
            assert m.any() and np.abs(flat["uv"][m][:, :2] - sol).max() < 1e-5
    else:
        # (no material of these scenes reads a texture and no mesh has coordinates: the frame hook reports 0, the field the barycentrics)
        assert not frame["uv"].any() and (flat["uv"][on][:, :2] >= 0).all() and (flat["uv"][on][:, :2].sum(1) <= 1 + 1e-6).all()


# ---- 3. primIndex ----
def test_prim_index_names_the_surface_the_position_lies_on():
    s = samples("hand")
    desc = hand_scene()
    F = {k: v.reshape(-1, 3) for k, v in s["fields"].items()}
    on = s["hit"]["prim"] >= 0
    prim, p = F["primIndex"][on][:, 0].astype(np.int64), F["position"][on].astype(np.float64)
    assert np.array_equal(F["primIndex"][on][:, 0], prim.astype(f32)) and np.array_equal(F["primIndex"][on][:, 1], F["primIndex"][on][:, 2])
    n_tris = len(desc.indices)
    pos = np.asarray(desc.positions, np.float64)
    bound = 1e-4 * (pos.max(0) - pos.min(0)).max()  # the project's ray epsilon times the scene's extent
    seen = set()
    for k, q in zip(prim, p):
        seen.add(int(k))
        if k < n_tris:
            a, b_, c_ = pos[desc.indices[k].astype(int)]
            n = np.cross(b_ - a, c_ - a); n /= np.linalg.norm(n)
            assert abs(np.dot(q - a, n)) <= bound
            for u, v in ((a, b_), (b_, c_), (c_, a)):  # inside every edge, by the same margin
                assert np.dot(np.cross(v - u, q - u), n) >= -bound * np.linalg.norm(v - u)
        elif k == n_tris:
            assert abs(np.linalg.norm(q - _slot_centre(SPHERE_SLOT)) - HALF) <= bound
        elif k == n_tris + 1:
            r = q - _slot_centre(DISK_SLOT)
            assert abs(r[2]) <= bound and np.hypot(r[0], r[1]) <= HALF + bound
        else:
            assert k == n_tris + 2
            local = (q - (_slot_centre(CYL_SLOT) - [CYL_LEN / 2, 0, 0])) @ CYL_ROT
            assert abs(np.hypot(local[0], local[1]) - CYL_R) <= bound and -bound <= local[2] <= CYL_LEN + bound
    assert {n_tris, n_tris + 1, n_tris + 2} <= seen and len(seen) >= 12
    # the triangle index is the scene description's, not the BVH's leaf order: on the room some hit's leaf-order index differs from it
    r = samples("room")
    ron = r["hit"]["prim"] >= 0
    assert (r["fields"]["primIndex"].reshape(-1, 3)[ron][:, 0].astype(np.int64) != r["hit"]["prim"][ron]).any()


# ---- 4. relPosition ----
@pytest.mark.parametrize("name", ["cbox", "hand", "lens"])
def test_rel_position_is_the_inverse_camera_transform(name):
    s = samples(name)
    on = s["hit"]["prim"] >= 0
    p = s["fields"]["position"].reshape(-1, 3)[on].astype(np.float64)
    c2w = np.asarray(_desc(name).camera["camera_to_world"], f32).reshape(4, 4).astype(np.float64)
    inv = np.linalg.inv(c2w)
    want = p @ inv[:3, :3].T + inv[:3, 3]
    bound = 6 * 2.0 ** -24 * (np.abs(p) @ np.abs(inv[:3, :3]).T + np.abs(inv[:3, 3]))
    got = s["fields"]["relPosition"].reshape(-1, 3)[on].astype(np.float64)
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()
    assert (got[:, 2] > 0).all()  # in front of the camera


# ---- 5. albedo ----
def _fdr(eta):
    """ppg_fresnel_diffuse_reflectance (include/ppg_detmath.h) in float64: composite Simpson, 4096 intervals, of F(sqrt(x), eta)"""
    def fresnel(ci):
        ct2 = 1.0 - (1.0 - ci * ci) * (1.0 / eta if ci > 0 else eta) ** 2
        if ct2 <= 0:
            return 1.0
        ct = np.sqrt(ct2)
        rs, rp = (ci - eta * ct) / (ci + eta * ct), (eta * ci - ct) / (eta * ci + ct)
        return 0.5 * (rs * rs + rp * rp)
    n, h = 4096, 1.0 / 4096
    acc = fresnel(0.0) + fresnel(1.0)
    for i in range(1, n):
        acc += (4.0 if i & 1 else 2.0) * fresnel(np.sqrt(i * h))
    return acc * h / 3.0


def test_albedo_by_bsdf_type():
    s = samples("hand")
    F = {k: v.reshape(-1, 3) for k, v in s["fields"].items()}
    on = s["hit"]["prim"] >= 0
    prim = np.where(on, F["primIndex"][:, 0], -1).astype(np.int64)
    n_tris = 2 * len(QUAD_SLOTS)
    slot = np.full(prim.shape, -1)
    for q, sl in enumerate(QUAD_SLOTS):
        slot[(prim == 2 * q) | (prim == 2 * q + 1)] = sl
    slot[prim == n_tris], slot[prim == n_tris + 1], slot[prim == n_tris + 2] = SPHERE_SLOT, DISK_SLOT, CYL_SLOT
    alb = F["albedo"]
    refl = lambda sl: np.asarray(MATERIALS[sl]["reflectance"], f32)  # noqa: E731
    for sl in range(11):
        assert (slot == sl).sum() >= 2, sl
    # constants come out exact: diffuse, roughdiffuse (sphere), phong (disk), twosided (cylinder), the normal-mapped quad, roughplastic
    # (its reflectance, without Ftr), the coated diffuse (its base)
    for sl in (1, 2, 3, 4, 5, 8, 10):
        assert np.array_equal(alb[slot == sl], np.broadcast_to(refl(sl), ((slot == sl).sum(), 3))), sl
    assert not alb[slot == 9].any()  # the conductor
    # the bitmapped quad: BitmapTexture::eval at the hit's uv, restated as tests/test_textures.py restates it, with its tolerance
    m = slot == 0
    want = _np_lookup(TEX, F["uv"][m][:, :2], (1, 1), (0, 0), ("repeat", "repeat"), False)
    assert np.abs(alb[m] - want).max() < 2e-3 and np.abs(alb[m] - want).mean() < 2e-5 and np.ptp(alb[m], axis=0).min() > 0.01
    # plastic: reflectance * (1 - fdrExt(eta)), in float64
    eta = float(f32(1.49))
    want = refl(7).astype(np.float64) * (1.0 - _fdr(eta))
    assert 0.85 < 1.0 - _fdr(eta) < 0.97
    assert ulps(alb[slot == 7], np.broadcast_to(want.astype(f32), ((slot == 7).sum(), 3))).max() <= 4
    # the mask: opacity texel (bilinear at the hit's uv) times the reflectance
    m = slot == 6
    op = _np_lookup(OPAC, F["uv"][m][:, :2], (1, 1), (0, 0), ("repeat", "repeat"), False).astype(np.float64)
    want = (op * refl(6).astype(np.float64)).astype(f32)
    assert ulps(alb[m], want).max() <= 2


def test_albedo_refuses_a_blended_scene_and_the_other_fields_render():
    from ppg_host.bindings import PPGError
    e = hip()
    e.set_scene(hand_scene(blend=True))
    with pytest.raises(PPGError, match="albedo: blendbsdf / mixturebsdf materials are not supported yet") as ex:
        e.render_fields(["shNormal", "albedo"])
    assert ex.value.code == -1
    got = e.render_fields(["shNormal"], undefined=[UNDEF[4]])["shNormal"]
    assert _same(got, samples("hand")["fields"]["shNormal"])
    e.close()


# ---- 6. filters ----
def np_fields_splat(V, rf, seed, first):
    """The documented order (j, dy, dx) in float32: V[j] = the per-sample values [h, w, c] of sample first + j (any number of channels: the
    weights do not depend on the field); -> (image, per pixel and channel sum |w V| / |sum w|).  For one sample and three channels this is
    np_splat's arithmetic (tests/test_rfilter_gpu.py)."""
    import ppg_host.bindings as b
    table, r, B = b.rfilter_table(rf)
    r, scale = f32(r), f32(31) / f32(r)
    H, W, nc = V[0].shape
    pix = np.arange(H * W, dtype=np.uint32)
    ty, tx = np.mgrid[0:H, 0:W]
    S, A = np.zeros((H, W, nc + 1), f32), np.zeros((H, W, nc), np.float64)
    for j, L in enumerate(V):
        posx = (((pix % W).astype(f32) + _rand(seed, pix, first + j, 0)) - f32(0.5)).reshape(H, W)
        posy = (((pix // W).astype(f32) + _rand(seed, pix, first + j, 1)) - f32(0.5)).reshape(H, W)
        for dy in range(-B, B + 1):
            for dx in range(-B, B + 1):
                sy, sx = ty - dy, tx - dx
                ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
                syc, sxc = np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)
                px, py = posx[syc, sxc], posy[syc, sxc]
                ylo = np.maximum(np.ceil(py - r).astype(np.int64), 0); yhi = np.minimum(np.floor(py + r).astype(np.int64), H - 1)
                xlo = np.maximum(np.ceil(px - r).astype(np.int64), 0); xhi = np.minimum(np.floor(px + r).astype(np.int64), W - 1)
                ok &= (ty >= ylo) & (ty <= yhi) & (tx >= xlo) & (tx <= xhi)
                wy = table[np.minimum(np.abs((ty.astype(f32) - py) * scale).astype(np.int64), 31)]
                wx = table[np.minimum(np.abs((tx.astype(f32) - px) * scale).astype(np.int64), 31)]
                w = wx * wy
                c = np.concatenate([w[..., None] * L[syc, sxc], w[..., None]], axis=2)
                S = S + np.where(ok[..., None], c, f32(0))
                A += np.where(ok[..., None], np.abs(c[..., :nc].astype(np.float64)), 0.0)
    nz = S[..., nc] != 0
    iw = np.where(nz, f32(1) / np.where(nz, S[..., nc], f32(1)), f32(0)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return S[..., :nc] * iw[..., None], np.where(nz[..., None], A / np.abs(S[..., nc:].astype(np.float64)), 0.0)


def _finite_samples(e, first, n):
    """the per-sample values [h, w, 3 * 8] of samples first .. first + n - 1, all fields side by side, with finite `undefined` values, from
    a box-filter engine (spp = 1: the image is the sample)"""
    return [np.concatenate(list(e.render_field_planes(ALL, spp=1, undefined=UNDEF_FINITE, first_sample=first + j)), axis=2) for j in range(n)]


@pytest.mark.parametrize("name", ["cbox", "hand"])
def test_filtered_fields_are_the_splat_in_the_documented_order(name):
    box = samples(name)["engine"]
    one, three = _finite_samples(box, 0, 1), _finite_samples(box, 2, 3)
    assert np.array_equal(np_fields_splat([one[0][..., :3]], FILTERS[0], SEED, 0)[0], np_splat(one[0][..., :3], FILTERS[0], SEED, 0))
    g = hip()
    g.set_scene(_desc(name))
    for rf in FILTERS:
        g.set_rfilter(rf)
        for V, spp, first in ((one, 1, 0), (three, 3, 2)):
            got = np.concatenate(list(g.render_field_planes(ALL, spp=spp, undefined=UNDEF_FINITE, first_sample=first)), axis=2)
            want, mag = np_fields_splat(V, rf, SEED, first)
            bad = ~(np.abs(got.astype(np.float64) - want) <= 2e-6 * mag)
            assert np.isfinite(got).all() and not bad.any(), (rf, spp, sorted({ALL[c // 3] for c in np.nonzero(bad)[2]}))
    g.close()
    # the default box with spp = 3: every pixel is the mean of its own three samples, summed in sample order
    got = box.render_fields(["position"], spp=3, undefined=[UNDEF_FINITE[0]], first_sample=2)["position"]
    acc = (three[0][..., :3] + three[1][..., :3]) + three[2][..., :3]
    assert np.array_equal(got, acc * (f32(1) / f32(3)))


# ---- 7. determinism ----
def test_fields_are_deterministic_and_a_shard_renders_the_whole_film():
    s = samples("hand")
    e = s["engine"]
    again = e.render_fields(ALL, spp=1, undefined=UNDEF)
    for k in ALL:
        assert again[k].tobytes() == s["fields"][k].tobytes(), k
    planes = e.render_field_planes(["albedo", "shNormal", "albedo", "uv", "shNormal"], spp=2, undefined=[9.0, 0.5, 9.0, -7.0, 0.5], first_sample=1)
    assert planes.shape == (5, HH, HW, 3)
    assert planes[0].tobytes() == planes[2].tobytes() and planes[1].tobytes() == planes[4].tobytes() and planes[0].tobytes() != planes[3].tobytes()
    for name in ("cbox", "hand"):
        ref = samples(name)
        sh = hip()
        sh.set_scene(_desc(name))
        sh.set_shard(1, 2)
        got = sh.render_fields(ALL, spp=1, undefined=UNDEF)
        for k in ALL:
            assert got[k].tobytes() == ref["fields"][k].tobytes(), (name, k)
        sh.close()


# ---- 8. the render is untouched ----
def test_a_render_is_bit_identical_with_and_without_the_fields():
    import ppg_host
    from ppg_host.bindings import Fields, PPGError
    desc = ppg_host.cbox_scene(67, 41)

    def render(before=False, after=False):
        e = hip(budget=8)
        e.set_scene(desc)
        if before:
            e.render_fields(ALL, spp=2)
        e.render()
        film = e.read_film()
        if after:
            e.render_fields(ALL, spp=2)
            assert film.tobytes() == e.read_film().tobytes()
        e.close()
        return film.tobytes()
    plain = render()
    assert plain == render(before=True) and plain == render(after=True) and np.frombuffer(plain, f32).mean() > 0
    e = hip(budget=8)
    e.set_scene(desc)
    e.begin_render()
    with pytest.raises(PPGError, match="ppg_render_fields: not between ppg_begin_render and ppg_end_render") as ex:
        e.render_fields(["albedo"])
    assert ex.value.code == -3
    with pytest.raises(PPGError, match="ppg_debug_camera_rays: not between ppg_begin_render and ppg_end_render"):
        e.debug_camera_rays()
    e.end_render()
    assert Fields is not None
    e.close()


# ---- 9. validation ----
def test_refusals_by_message():
    from ppg_host.bindings import Fields, PPGError
    e = hip()
    out = np.zeros((8, 13, 17, 3), f32)
    ptr = out.ctypes.data_as(C.POINTER(C.c_float))

    def call(f, o=ptr):
        rc = e.lib.ppg_render_fields(e.ctx, C.byref(f) if f is not None else None, o)
        return rc, e.lib.ppg_last_error(e.ctx).decode()
    f = Fields()
    f.n_fields, f.spp = 1, 1
    assert call(f) == (-3, "no scene")
    e.set_scene(hand_scene())
    assert call(None)[0] == -1 and "no fields or no output" in call(None)[1]
    assert call(f, None)[0] == -1 and "no fields or no output" in call(f, None)[1]
    for n in (0, 9):
        f.n_fields = n
        assert call(f) == (-1, "ppg_render_fields: n_fields must be 1 .. 8")
    f.n_fields = 2
    for bad in (8, -1):
        f.field[1] = bad
        rc, msg = call(f)
        assert rc == -1 and "field 1: unknown field %d" % bad in msg
    f.field[1] = 6
    for spp in (0, 65537):
        f.spp = spp
        assert call(f) == (-1, "ppg_render_fields: spp must be 1 .. 65536")
    f.spp = 1
    assert call(f)[0] == 0 and not out[2:].any() and out[1].any()
    with pytest.raises(ValueError, match="position, relPosition, distance, geoNormal, shNormal, uv, albedo, primIndex"):
        e.render_fields(["shapeIndex"])
    e.close()
