"""Analytic disks and cylinders on the GPU (include/ppg.h ppg_set_shapes; ppg_device.h shape_hit, fill_isect_shape, shape_sample_direct).
The CPU oracle does not know these shapes, so nothing here is "GPU equals oracle":

  * ray by ray and sample by sample through the two test hooks (include/ppg_testhooks.h) against float64 restatements of the ray tests, the
    intersection records and the area sampling of Mitsuba's disk and cylinder plug-ins,
  * the film of a scene in which the shapes are seen directly against a restatement of every primary ray,
  * statistically, with bounces, MIS and guiding, against flat-shaded 128-sided meshes of equal area,
  * and the host paths (determinism, sharding, the C++ driver, the scene box, clearing the list, the refusals).

Bounds.  A device result is the end of about 40 rounded float32 operations (ray to object space, the root, the point, its way back, the
frame): 40 x 6e-8 = 2.4e-6 relative; the bound is B = 2e-5, ten times that (tests/test_delta_emitters_gpu.py derives its 2e-5 the same way).
A root's sensitivity to its inputs is 1 / |cos| of the angle of incidence, so positions are compared to B * scale / |cos| with scale = the
size of the numbers involved (1 + |o| + t), and unit vectors derived from a position to that divided by the length they are normalised
by.  Rays whose answer depends on less than 1e-4 of a shape's size (rim, end circles, tangency), or on a root within 2e-5 of mint / maxt,
are not compared: the batches are built so that they are few, and the tests assert that."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import IMPROVED, ROOT
from test_rfilter_gpu import _rand
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu

B = 2e-5
EPS = 1e-4  # PPG_EPSILON: the render's ray epsilon, scaled by the largest coordinate of the origin
W, H = 48, 40


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


# ---------------------------------------------------------------------------------------------- the shapes
def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _disk(center, radius, R, flip=False, **kw):
    m = np.concatenate([R * radius, np.asarray(center, np.float64)[:, None]], 1)
    return dict(type="disk", to_world=[float(f32(v)) for v in m.reshape(-1)], flip_normals=flip, **kw)


def _cylinder(base, R, radius, length, flip=False, **kw):
    m = np.concatenate([R, np.asarray(base, np.float64)[:, None]], 1)
    return dict(type="cylinder", to_world=[float(f32(v)) for v in m.reshape(-1)], radius=float(f32(radius)), length=float(f32(length)), flip_normals=flip, **kw)


CAM_O = (0.0, 0.0, 3.2)
QUAD_Z = -1.5
RADIANCE = [(1.0, 2.0, 3.0), (2.5, 0.5, 1.5), (0.75, 1.25, 0.25), (3.0, 3.5, 1.0)]
SHAPES = [
    _disk((-0.95, 0.55, 0.0), 0.8, _rot((1, 0, 0), 30)),                                        # radius 0.8, tilted 30 degrees
    _disk((1.0, 0.85, 0.3), 0.55, _rot((0, 1, 0), 20) @ _rot((1, 0, 0), -25), flip=True),       # flipped: its back faces the camera
    _cylinder((-0.75, -0.95, 0.0), _rot((0.3, 1.0, 0.0), 17), 0.3, 1.2),                         # oblique axis, open end towards the camera
    _cylinder((0.8, -0.75, 0.4), _rot((1.0, -0.4, 0.0), 14), 0.33, 1.0, flip=True),              # flipped: the inside emits
]


def _scene(emitters=True):
    """the four shapes in front of a black quad (two triangles) at z = -1.5; with emitters=True each shape is an area emitter"""
    import ppg_host
    pos = np.array([(-3, -3, QUAD_Z), (3, -3, QUAD_Z), (3, 3, QUAD_Z), (-3, 3, QUAD_Z)], f32)
    idx = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
    cam = ppg_host.scenes.perspective_camera(CAM_O, (0.0, 0.0, 0.0), (0, 1, 0), 60.0, "x", 0.01, 100.0, W, H)
    shapes = [dict(s, material=1 + (k & 1), emitter=k if emitters else -1) for k, s in enumerate(SHAPES)]
    mats = [dict(type=0, reflectance=(0.0, 0.0, 0.0)), dict(type=0, reflectance=(0.5, 0.5, 0.5)), dict(type=0, reflectance=(0.2, 0.3, 0.4))]
    return ppg_host.SceneDesc(pos, idx, np.zeros(2, np.uint32), np.full(2, -1, np.int32), mats,
                              [dict(radiance=r) for r in RADIANCE] if emitters else [], cam, shapes=shapes)


class Shape64:
    """a ppg_shape record in float64: the float32 matrix as the library receives it, its exact inverse, and what the plug-ins derive"""

    def __init__(self, rec):
        self.cyl = rec["type"] == "cylinder"
        m = np.asarray(rec["to_world"], np.float64).reshape(3, 4)
        self.L, self.T = m[:, :3], m[:, 3]
        self.Li = np.linalg.inv(self.L)
        self.flip = bool(rec.get("flip_normals"))
        self.r = float(rec["radius"]) if self.cyl else 1.0
        self.len = float(rec["length"]) if self.cyl else 0.0
        self.size = min(self.r, self.len) if self.cyl else float(np.linalg.norm(self.L[:, 0]))   # world length of the smallest feature
        self.inv_area = 1 / (2 * math.pi * self.r * self.len) if self.cyl else 1 / (math.pi * np.linalg.norm(self.L[:, 0]) ** 2)

    def to_obj(self, p):
        return (p - self.T) @ self.Li.T

    def vec_to_obj(self, v):
        return v @ self.Li.T

    def normal_to_world(self, n):  # the transposed inverse, normalised
        w = n @ self.Li
        return w / np.linalg.norm(w, axis=-1, keepdims=True)

    def intersect(self, o, d, mint, maxt, any_hit):
        """t[n] (inf = no hit) and unsure[n] by the plug-in's rayIntersect (any_hit: its form without t), the ray taken to object space"""
        lo, ld = self.to_obj(o), self.vec_to_obj(d)
        n = len(o)
        t, unsure = np.full(n, np.inf), np.zeros(n, bool)
        with np.errstate(all="ignore"):
            if not self.cyl:
                hit = -lo[:, 2] / ld[:, 2]
                in_range = (hit >= mint) & (hit <= maxt)
                x, y = lo[:, 0] + ld[:, 0] * hit, lo[:, 1] + ld[:, 1] * hit
                r = np.hypot(x, y)
                ok = in_range & (r * r <= 1)
                t[ok] = hit[ok]
                rt = B * np.maximum(1.0, np.abs(hit))
                near_range = (np.abs(hit - mint) < rt) | (np.abs(hit - maxt) < rt)
                # (a ray almost in the plane: the float32 error of its object z, 2e-7, moves the point along the ray)
                err_r = 2e-7 / np.abs(ld[:, 2]) * np.abs(hit) * np.hypot(ld[:, 0], ld[:, 1]) + 1e-6
                unsure = np.isfinite(hit) & ((near_range & (r <= 1 + 1e-4)) | ((in_range | near_range) & (np.abs(r - 1) < np.maximum(1e-4, 4 * err_r))))
                unsure |= (np.abs(ld[:, 2]) < 1e-6 * np.linalg.norm(ld, axis=1)) & (np.abs(lo[:, 2]) < 1e-4)
                # (... but a ray that far off the plane meets it, whatever its object z is within 2e-7, well outside the disk: a sure miss)
                lxy, oxy = np.hypot(ld[:, 0], ld[:, 1]), np.hypot(lo[:, 0], lo[:, 1])
                unsure &= ~(np.abs(lo[:, 2]) / (np.abs(ld[:, 2]) + 2e-7) * lxy - oxy > 2)
                return t, unsure
            ox, oy, dx, dy = lo[:, 0], lo[:, 1], ld[:, 0], ld[:, 1]
            A, Bq, Cq = dx * dx + dy * dy, 2 * (dx * ox + dy * oy), ox * ox + oy * oy - self.r * self.r
            parallel = A < 1e-10 * np.sum(ld * ld, 1)
            disc = Bq * Bq - 4 * A * Cq
            sq = np.sqrt(np.maximum(disc, 0))
            temp = np.where(Bq < 0, -0.5 * (Bq - sq), -0.5 * (Bq + sq))
            x0, x1 = temp / A, Cq / temp
            near, far = np.minimum(x0, x1), np.maximum(x0, x1)
            solved = ~parallel & (disc >= 0)
            in_range = ((near <= maxt) & (far >= mint)) if not any_hit else ~((near > maxt) | (far < mint))
            zn, zf = lo[:, 2] + ld[:, 2] * near, lo[:, 2] + ld[:, 2] * far
            take_near = (zn >= 0) & (zn <= self.len) & (near >= mint)
            take_far = ~take_near & (zf >= 0) & (zf <= self.len) & (far <= maxt)
            ok_n, ok_f = solved & in_range & take_near, solved & in_range & take_far
            t[ok_n] = near[ok_n]
            t[ok_f] = far[ok_f]
            # margins: tangency (the distance of the line from the axis against the radius), the end circles, the range
            rho = np.sqrt(np.maximum(ox * ox + oy * oy - (0.5 * Bq) ** 2 / A, 0))
            unsure = ~parallel & (np.abs(rho - self.r) < 1e-4 * self.r)
            for root, z in ((near, zn), (far, zf)):
                rt = B * np.maximum(1.0, np.abs(root))
                live = solved & (root >= mint - rt) & (root <= maxt + rt)
                unsure |= live & ((np.abs(z) < 1e-4 * self.len) | (np.abs(z - self.len) < 1e-4 * self.len))
                unsure |= solved & (z >= -1e-4 * self.len) & (z <= self.len * (1 + 1e-4)) & ((np.abs(root - mint) < rt) | (np.abs(root - maxt) < rt))
            unsure |= parallel & (np.abs(np.hypot(ox, oy) - self.r) < 1e-4 * self.r)
        return t, unsure

    def record(self, o, d, t):
        """p, n, s, |cos| of the incidence and the length the tangent is normalised by, by the plug-in's fillIntersectionRecord"""
        p = o + d * t[:, None]
        local = self.to_obj(p)
        x, y = local[:, 0], local[:, 1]
        r = np.hypot(x, y)
        if not self.cyl:
            n = np.broadcast_to(self.normal_to_world(np.array([0.0, 0.0, 1.0])), p.shape).copy()
            with np.errstate(all="ignore"):
                du = np.where((r != 0)[:, None], np.stack([x / r, y / r, np.zeros_like(x)], 1), np.array([1.0, 0.0, 0.0]))
            dpdu = du @ self.L.T
            tangent_len = r * self.size
        else:
            dpdu = np.stack([-y, x, np.zeros_like(x)], 1) * (2 * math.pi) @ self.L.T
            dpdv = np.array([0.0, 0.0, self.len]) @ self.L.T
            gs = dpdu / np.linalg.norm(dpdu, axis=1, keepdims=True)
            n = np.cross(gs, dpdv / np.linalg.norm(dpdv))
            p = p + n * (self.r - r)[:, None]
            tangent_len = np.full(len(p), self.r)
        if self.flip:
            n = -n
        s = dpdu - n * np.sum(n * dpdu, 1, keepdims=True)
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        cos = np.abs(np.sum(n * d, 1)) / np.linalg.norm(d, axis=1)
        return p, n, s, cos, tangent_len


def _quad(o, d, mint, maxt):
    """the two triangles behind the shapes: t, unsure, the normal"""
    with np.errstate(all="ignore"):
        t = (QUAD_Z - o[:, 2]) / d[:, 2]
        x, y = o[:, 0] + d[:, 0] * t, o[:, 1] + d[:, 1] * t
        inside = (np.abs(x) <= 3) & (np.abs(y) <= 3) & (t >= mint) & (t <= maxt)
        rt = B * np.maximum(1.0, np.abs(t))
        unsure = np.isfinite(t) & ((np.abs(np.abs(x) - 3) < 6e-4) | (np.abs(np.abs(y) - 3) < 6e-4) | (np.abs(t - mint) < rt) | (np.abs(t - maxt) < rt))
        unsure &= (np.abs(x) <= 3.001) & (np.abs(y) <= 3.001)
    return np.where(inside, t, np.inf), unsure


def _closest(shapes, o, d, mint, maxt, any_hit=False):
    """the closest primitive in float64: kind[n] (-1 none, 0 the quad, 1 + k shape k), t[n], unsure[n]"""
    ts, un = zip(*([_quad(o, d, mint, maxt)] + [s.intersect(o, d, mint, maxt, any_hit) for s in shapes]))
    ts, unsure = np.stack(ts), np.any(un, 0)
    kind = np.argmin(ts, 0)
    t = ts[kind, np.arange(ts.shape[1])]
    srt = np.sort(ts, 0)
    with np.errstate(invalid="ignore"):
        unsure |= np.isfinite(srt[1]) & (srt[1] - srt[0] < B * np.maximum(1.0, srt[0]))  # two primitives at (almost) the same distance
    return np.where(np.isfinite(t), kind, -1), t, unsure


# ---------------------------------------------------------------------------------------------- 1. ray by ray
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _ray_batch(shapes, rng):
    """4096 rays (o, mint, d, maxt) in float32 and the class of each"""
    disk, cyl = shapes[0], shapes[2]
    rays, cls = [], []

    def add(name, o, d, mint=None, maxt=None):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        n = len(o)
        mint = np.full(n, EPS) if mint is None else mint
        maxt = np.full(n, np.inf) if maxt is None else maxt
        rays.append(np.concatenate([o, np.asarray(mint)[:, None], d, np.asarray(maxt)[:, None]], 1))
        cls.extend([name] * n)

    def on_cyl(c, n, z=None):
        phi = rng.uniform(0, 2 * math.pi, n)
        z = rng.uniform(0.05, 0.95, n) * c.len if z is None else z
        return np.stack([c.r * np.cos(phi), c.r * np.sin(phi), z], 1), phi

    def world(s, p):
        return p @ s.L.T + s.T

    # random rays from outside, aimed into the scene
    n = 1100
    o = rng.uniform(-2.5, 2.5, (n, 3)); o[:, 2] = rng.uniform(2.0, 4.0, n)
    tgt = rng.uniform(-1.6, 1.6, (n, 3)); tgt[:, 2] = rng.uniform(-0.5, 1.0, n)
    add("outside", o, _unit(tgt - o))
    # from inside the cylinders
    for c in (shapes[2], shapes[3]):
        n = 250
        phi, rad = rng.uniform(0, 2 * math.pi, n), c.r * np.sqrt(rng.uniform(0, 0.9, n))
        o = world(c, np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(0.1, 0.9, n) * c.len], 1))
        add("inside", o, _unit(rng.normal(size=(n, 3))))
    # entering through an open end: from beyond an end, aimed at a point of the wall inside
    for c in (shapes[2], shapes[3]):
        for end in (0, 1):
            n = 125
            phi, rad = rng.uniform(0, 2 * math.pi, n), 0.6 * c.r * np.sqrt(rng.uniform(0, 1, n))
            zo = -rng.uniform(0.2, 0.8, n) if end == 0 else c.len + rng.uniform(0.2, 0.8, n)
            o = world(c, np.stack([rad * np.cos(phi), rad * np.sin(phi), zo], 1))
            tgt, _ = on_cyl(c, n, rng.uniform(0.25, 0.75, n) * c.len)
            add("open end", o, _unit(world(c, tgt) - o))
    # parallel to the disks' planes (object d.z = 0), off the plane
    for s in (shapes[0], shapes[1]):
        n = 150
        phi = rng.uniform(0, 2 * math.pi, n)
        o = world(s, np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.choice([-1, 1], n) * rng.uniform(0.05, 0.6, n)], 1))
        add("in plane", o, _unit(np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], 1) @ s.L.T))
    # along the cylinders' axes (A = 0), inside and outside the tube
    for c in (shapes[2], shapes[3]):
        n = 150
        phi, rad = rng.uniform(0, 2 * math.pi, n), c.r * rng.choice([0.5, 1.7], n) * rng.uniform(0.5, 1.0, n)
        o = world(c, np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(-1, 2, n)], 1))
        add("along axis", o, np.tile(c.L[:, 2] * rng.choice([-1, 1]), (n, 1)))
    # aimed at the rims of the disks and the end circles of the cylinders: within +-3 % of the radius around them
    for s in shapes:
        n = 120
        phi, rad = rng.uniform(0, 2 * math.pi, n), s.r * (1 + rng.uniform(-0.03, 0.03, n))
        z = rng.choice([0.0, s.len], n) + (rng.uniform(-0.03, 0.03, n) * s.len if s.cyl else 0)
        tgt = world(s, np.stack([rad * np.cos(phi), rad * np.sin(phi), z], 1))
        o = np.asarray(CAM_O) + rng.uniform(-1.5, 1.5, (n, 3))
        add("rim", o, _unit(tgt - o))
    # maxt between a cylinder's two roots: through the wall (the near root counts) and through an open end (nothing counts)
    for c in (shapes[2], shapes[3]):
        n = 110
        a, _ = on_cyl(c, n)
        b_, _ = on_cyl(c, n)
        d = _unit(world(c, b_) - world(c, a))
        o = world(c, a) - d * rng.uniform(0.5, 1.5, n)[:, None]
        chord = np.linalg.norm(world(c, b_) - world(c, a), axis=1)
        add("maxt between", o, d, maxt=np.linalg.norm(world(c, a) - o, axis=1) + chord * rng.uniform(0.2, 0.8, n))
        phi, rad = rng.uniform(0, 2 * math.pi, n), 0.5 * c.r * np.sqrt(rng.uniform(0, 1, n))
        o = world(c, np.stack([rad * np.cos(phi), rad * np.sin(phi), -rng.uniform(0.3, 0.8, n)], 1))
        tgt, _ = on_cyl(c, n, rng.uniform(0.3, 0.7, n) * c.len)
        dist = np.linalg.norm(world(c, tgt) - o, axis=1)
        add("maxt between", o, _unit(world(c, tgt) - o), maxt=dist * rng.uniform(0.5, 0.9, n))
    # starting on a shape with the render's epsilon
    for s in shapes:
        n = 110
        if s.cyl:
            p, _ = on_cyl(s, n)
        else:
            phi, rad = rng.uniform(0, 2 * math.pi, n), np.sqrt(rng.uniform(0, 0.8, n))
            p = np.stack([rad * np.cos(phi), rad * np.sin(phi), np.zeros(n)], 1)
        o = world(s, p).astype(f32).astype(np.float64)
        add("on a shape", o, _unit(rng.normal(size=(n, 3))), mint=EPS * np.maximum(np.abs(o).max(1), EPS))
    rays = np.concatenate(rays).astype(f32)
    assert len(rays) <= 4096
    n = 4096 - len(rays)
    o = rng.uniform(-2.5, 2.5, (n, 3)); o[:, 2] = rng.uniform(2.0, 4.0, n)
    extra = np.concatenate([o, np.full((n, 1), EPS), _unit(rng.uniform(-1.5, 1.5, (n, 3)) - o), np.full((n, 1), np.inf)], 1).astype(f32)
    return np.concatenate([rays, extra]), np.array(cls + ["outside"] * n)


CLASSES = ("outside", "inside", "open end", "in plane", "along axis", "rim", "maxt between", "on a shape")


@pytest.mark.parametrize("any_hit", [False, True])
def test_rays_equal_the_restatement(any_hit):
    desc = _scene()
    shapes = [Shape64(s) for s in desc.shapes]
    rays, cls = _ray_batch(shapes, np.random.default_rng(7))
    assert rays.shape == (4096, 8)
    e = hip(budgetType="spp", budget=4)
    e.set_scene(desc)
    got = e.debug_intersect(rays, any_hit=any_hit)
    e.close()
    r64 = rays.astype(np.float64)
    o, d, mint, maxt = r64[:, :3], r64[:, 4:7], r64[:, 3], r64[:, 7]
    kind, t, unsure = _closest(shapes, o, d, mint, maxt, any_hit)
    counted = ~unsure
    print("%s: rays left out %d of 4096; per class counted / hits: %s" % (
        "any-hit" if any_hit else "closest-hit", unsure.sum(), {c: (int((counted & (cls == c)).sum()), int((counted & (cls == c) & (kind > 0)).sum())) for c in CLASSES}))
    assert unsure.sum() <= 0.02 * 4096
    for c in CLASSES:
        assert (counted & (cls == c)).sum() >= 50, c
    # what the classes are for
    assert (kind[counted & (cls == "in plane")] != 1).all() and (kind[counted & (cls == "in plane")] != 2).any()
    assert ((kind > 0) & counted & (cls == "open end")).sum() >= 50 and ((kind > 0) & counted & (cls == "on a shape")).sum() >= 50
    for k in range(4):
        assert ((kind == 1 + k) & counted).sum() >= 100, k
    m = counted & (cls == "maxt between")
    assert ((kind >= 3) & m).sum() >= 50 and ((kind < 3) & m).sum() >= 50   # the near root counts / neither root does
    gp = got["prim"]
    if any_hit:
        bad = counted & ((gp >= 0) != (kind >= 0))
        assert not bad.any(), (np.argwhere(bad)[:10].ravel(), cls[bad][:10])
        return
    want_prim = np.where(kind > 0, 2 + kind - 1, np.where(kind == 0, 0, -1))
    is_tri = kind == 0
    bad = counted & np.where(is_tri, (gp < 0) | (gp > 1), gp != want_prim)
    assert not bad.any(), (np.argwhere(bad)[:10].ravel(), cls[bad][:10], gp[bad][:10], want_prim[bad][:10])
    worst = {}
    for k, s in enumerate(shapes):
        sel = counted & (kind == 1 + k)
        p, n, sv, cos, tlen = s.record(o[sel], d[sel], t[sel])
        scale = 1 + np.abs(o[sel]).max(1) + t[sel]
        tol = B * scale / np.maximum(cos, 1e-3)
        g = got[sel]
        err = dict(t=np.abs(g["t"] - t[sel]) / tol, p=np.abs(g["p"] - p).max(1) / tol, n=np.abs(g["n"] - n).max(1) / (tol / s.size + B),
                   geo_n=np.abs(g["geo_n"] - n).max(1) / (tol / s.size + B))
        with np.errstate(divide="ignore"):
            err["s"] = np.abs(g["s"] - sv).max(1) / (tol / np.maximum(tlen, 1e-30) + B)
        if not s.cyl:
            err["s"] = np.where(tlen > 1e-3 * s.size, err["s"], 0.0)  # (at the centre the radial direction is undefined)
        wi = np.stack([-(d[sel] * sv).sum(1), -(d[sel] * np.cross(n, sv)).sum(1), -(d[sel] * n).sum(1)], 1)
        err["wi"] = np.abs(g["wi"] - wi).max(1) / (2 * (tol / np.minimum(s.size, np.maximum(tlen, 1e-30)) + B))
        if not s.cyl:
            err["wi"] = np.where(tlen > 1e-3 * s.size, err["wi"], 0.0)
        worst[k] = {key: float(v.max()) for key, v in err.items()}
        assert (g["material"] == desc.shapes[k]["material"]).all() and (g["emitter"] == desc.shapes[k]["emitter"]).all()
    print("closest-hit: largest error / bound per shape:", worst)
    for k in worst:
        assert max(worst[k].values()) <= 1.0, (k, worst[k])
    sel = counted & is_tri
    assert np.abs(got["t"][sel] - t[sel]).max() <= B * (1 + np.abs(o[sel]).max() + t[sel].max())
    assert np.abs(got["n"][sel] - np.array([0.0, 0.0, 1.0])).max() <= B and (got["emitter"][sel] == -1).all() and (got["material"][sel] == 0).all()


# ---------------------------------------------------------------------------------------------- 2. sample by sample
def _concentric(u):
    """the concentric map of the unit square onto the unit disk (Shirley & Chiu)"""
    r1, r2 = 2 * u[:, 0] - 1, 2 * u[:, 1] - 1
    with np.errstate(all="ignore"):
        a = np.abs(r1) > np.abs(r2)
        r = np.where(a, r1, r2)
        phi = np.where(a, (math.pi / 4) * (r2 / r1), (math.pi / 2) - (r1 / r2) * (math.pi / 4))
    phi = np.where((r1 == 0) & (r2 == 0), 0.0, phi)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], 1)


def test_direct_samples_equal_the_restatement():
    import ppg_host
    desc = _scene(False)
    desc.shapes = [dict(desc.shapes[0], emitter=0), dict(desc.shapes[3], emitter=1)]   # the disk; the flipped cylinder (its inside emits)
    desc.emitters = [dict(radiance=RADIANCE[0]), dict(radiance=RADIANCE[3])]
    shapes = [Shape64(s) for s in desc.shapes]
    rng = np.random.default_rng(11)
    n = 4096
    u = rng.uniform(0, 1, (n, 2))
    u[:, 0] = np.clip(u[:, 0], 0.001, 0.999) + np.where(np.abs(u[:, 0] - 0.5) < 0.001, 0.002, 0.0)  # (off the ends of the cylinder by more than float rounding)
    u = u.astype(f32)
    ref = rng.uniform(-2.0, 2.0, (n, 3))
    cyl, disk = shapes[1], shapes[0]
    k = n // 4
    phi, rad = rng.uniform(0, 2 * math.pi, k), cyl.r * np.sqrt(rng.uniform(0, 0.8, k))
    ref[:k] = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(0.05, 0.95, k) * cyl.len], 1) @ cyl.L.T + cyl.T   # inside the cylinder
    ref[k:2 * k] = (rng.uniform(-1.5, 1.5, (k, 3)) * (1, 1, 0) + (0, 0, 1) * -rng.uniform(0.1, 1.5, k)[:, None]) @ disk.L.T / disk.size + disk.T  # behind the disk
    ref[2 * k:3 * k] = (rng.uniform(-1.5, 1.5, (k, 3)) * (1, 1, 0) + (0, 0, 1) * rng.uniform(0.1, 1.5, k)[:, None]) @ disk.L.T / disk.size + disk.T  # in front of it
    ref = ref.astype(f32)
    ref_n = _unit(rng.normal(size=(n, 3)))
    toward = _unit(np.where((u[:, :1] < 0.5), disk.T, cyl.T + cyl.L[:, 2] * cyl.len / 2) - ref)
    ref_n = np.where((rng.uniform(size=n) < 0.6)[:, None], toward, ref_n).astype(f32)
    e = hip(budgetType="spp", budget=4)
    e.set_scene(desc)
    got = e.debug_sample_direct(ref, ref_n, u)
    e.close()
    u64, r64, n64 = u.astype(np.float64), ref.astype(np.float64), ref_n.astype(np.float64)
    em = (u64[:, 0] >= 0.5).astype(int)
    sx, sy = 2 * u64[:, 0] - em, u64[:, 1]          # the emitter choice re-uses the sample: exact in float32 for two emitters
    assert (got["emitter"] == em).all() and (got["em_pdf"] == 0.5).all()
    pd = _concentric(np.stack([sx, sy], 1))
    p_disk = np.stack([pd[:, 0], pd[:, 1], np.zeros(n)], 1) @ disk.L.T + disk.T
    n_disk = np.broadcast_to(disk.normal_to_world(np.array([0.0, 0.0, 1.0])), (n, 3))
    ang = 2 * math.pi * sy
    p_cyl = np.stack([cyl.r * np.cos(ang), cyl.r * np.sin(ang), sx * cyl.len], 1) @ cyl.L.T + cyl.T
    n_cyl = -cyl.normal_to_world(np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1))   # flipped
    p = np.where(em[:, None] == 0, p_disk, p_cyl)
    nn = np.where(em[:, None] == 0, n_disk, n_cyl)
    dv = p - r64
    dist = np.linalg.norm(dv, axis=1)
    dv /= dist[:, None]
    dn, dr = (dv * nn).sum(1), (dv * n64).sum(1)
    inv_area = np.where(em == 0, disk.inv_area, cyl.inv_area)
    pdf = inv_area * dist ** 2 / np.abs(dn)
    lit = (dr >= 0) & (dn < 0)
    unsure = (np.abs(dn) < 1e-4) | (np.abs(dr) < 1e-4)
    ok = ~unsure
    # the point the device chose lies on the shape
    gp = r64 + got["d"].astype(np.float64) * got["dist"].astype(np.float64)[:, None]
    lo_d, lo_c = disk.to_obj(gp), cyl.to_obj(gp)
    on_disk = (np.abs(lo_d[:, 2]) <= 1e-5) & (lo_d[:, 0] ** 2 + lo_d[:, 1] ** 2 <= 1 + 1e-5)
    on_cyl = (np.abs(np.hypot(lo_c[:, 0], lo_c[:, 1]) / cyl.r - 1) <= 1e-5) & (lo_c[:, 2] >= 0) & (lo_c[:, 2] <= cyl.len)
    assert np.where(em == 0, on_disk, on_cyl).all()
    scale = 1 + np.abs(r64).max(1) + dist
    errs = dict(n=np.abs(got["n"] - nn).max(1) / B, d=np.abs(got["d"] - dv).max(1) / (B * scale / dist), dist=np.abs(got["dist"] - dist) / (B * scale))
    rad = np.where(em[:, None] == 0, np.asarray(RADIANCE[0]), np.asarray(RADIANCE[3]))
    tol_pdf = B * pdf * (2 + scale / dist + 1 / np.abs(dn))
    sel = ok & lit
    errs["pdf"] = np.where(sel, np.abs(got["pdf"] - pdf) / tol_pdf, 0)
    errs["value"] = np.where(sel[:, None], np.abs(got["value"] - rad / pdf[:, None]) / (rad * (tol_pdf / pdf ** 2)[:, None]), 0).max(1)
    print("direct samples: left out %d; lit %d, dark %d (disk %d / %d, cylinder %d / %d); largest error / bound: %s" % (
        unsure.sum(), (ok & lit).sum(), (ok & ~lit).sum(), (ok & lit & (em == 0)).sum(), (ok & ~lit & (em == 0)).sum(), (ok & lit & (em == 1)).sum(),
        (ok & ~lit & (em == 1)).sum(), {k_: float(v.max()) for k_, v in errs.items()}))
    assert unsure.sum() <= 0.02 * n
    for cls_em in (0, 1):
        assert (ok & lit & (em == cls_em)).sum() >= 200 and (ok & ~lit & (em == cls_em)).sum() >= 200
    dark = ok & ~lit
    assert (got["value"][dark] == 0).all() and (got["pdf"][dark] == 0).all()
    assert (got["pdf"][sel] > 0).all()
    for k_, v in errs.items():
        assert v.max() <= 1.0, k_


# ---------------------------------------------------------------------------------------------- 3. seen directly
SEED = 31


def _seen_directly(desc, shapes, spp=16):
    """per pixel: the sum over its samples of the radiance seen (float64 [H, W, 3]) / spp, whether a sample is within the margins of a
    silhouette, and per sample what it met: kind (as _closest) and whether it met the front"""
    cam = desc.camera
    s2c, c2w = np.asarray(cam["sample_to_camera"], np.float64), np.asarray(cam["camera_to_world"], np.float64)
    pix = np.arange(W * H, dtype=np.uint32)
    total, grazing = np.zeros((W * H, 3)), np.zeros(W * H, bool)
    n_front = np.zeros((5, W * H), np.int32)
    n_back = np.zeros((5, W * H), np.int32)
    n_unsure = 0
    for s in range(spp):
        sx, sy = (pix % W) + _rand(SEED, pix, s, 0).astype(np.float64), (pix // W) + _rand(SEED, pix, s, 1).astype(np.float64)
        q = s2c @ np.stack([sx / W, sy / H, np.zeros_like(sx), np.ones_like(sx)])
        d = q[:3] / q[3]
        d = (c2w[:3, :3] @ (d / np.linalg.norm(d, axis=0))).T
        o = np.broadcast_to(c2w[:3, 3], d.shape)
        mint = np.full(len(d), EPS * np.abs(o[0]).max())
        kind, t, unsure = _closest(shapes, o, d, mint, np.full(len(d), np.inf))
        n_unsure += int(unsure.sum())
        grazing |= unsure
        for k, sh in enumerate(shapes):
            sel = kind == 1 + k
            _, n, _, _, _ = sh.record(o[sel], d[sel], t[sel])
            front = (n * -d[sel]).sum(1) > 0
            grazing[np.flatnonzero(sel)[np.abs((n * d[sel]).sum(1)) < 1e-4]] = True
            total[np.flatnonzero(sel)[front]] += np.asarray(RADIANCE[k])
            np.add.at(n_front[1 + k], np.flatnonzero(sel)[front], 1)
            np.add.at(n_back[1 + k], np.flatnonzero(sel)[~front], 1)
    return (total / spp).reshape(H, W, 3), grazing.reshape(H, W), n_front.reshape(5, H, W), n_back.reshape(5, H, W), n_unsure


@pytest.mark.parametrize("env", ["", "PPG_FORCE_BVH"])
def test_shapes_seen_directly_equal_the_restatement_of_every_primary_ray(monkeypatch, env):
    """maxDepth = 1, emitters visible: a pixel is radiance x (its samples whose primary ray meets a front face first) / 16.  The sums of at
    most 16 equal radiances and the division by the weight are exact or one rounding each: the bound is 4 ulp."""
    if env:
        monkeypatch.setenv(env, "1")
    desc = _scene()
    shapes = [Shape64(s) for s in desc.shapes]
    e = hip(budgetType="spp", budget=16, sppPerPass=16, nee="never", maxDepth=1, hideEmitters=0, seed=SEED)
    e.set_scene(desc)
    e.render()
    film = e.read_film().astype(np.float64)
    e.close()
    want, grazing, n_front, n_back, n_unsure = _seen_directly(desc, shapes)
    whole = lambda a: int((a == 16).sum())  # noqa: E731
    print("seen directly%s: samples within a margin %d of %d, pixels left out %d of %d; whole pixels front / back per shape: %s" % (
        " (bvh)" if env else "", n_unsure, 16 * W * H, grazing.sum(), W * H, [(whole(n_front[1 + k]), whole(n_back[1 + k])) for k in range(4)]))
    assert grazing.sum() <= 0.01 * W * H
    assert whole(n_front[1]) >= 20                      # lit: the disk's front
    assert whole(n_back[2]) >= 20                       # a dark back face: the flipped disk
    assert whole(n_front[4]) >= 20                      # a visible interior: the flipped cylinder's
    assert whole(n_back[3]) >= 20                       # a dark one: the other cylinder's
    assert whole(n_front[3]) >= 20 and whole(n_back[4]) >= 20   # ... whose outside is lit; the flipped one's is dark
    ok = ~grazing
    err = np.abs(film - want) / (4 * 6e-8 * np.maximum(want, 1e-30))
    assert (film[ok][want[ok] == 0] == 0).all()
    assert (err[ok][want[ok] > 0] <= 1).all(), np.argwhere(ok[..., None] & (want > 0) & (err > 1))[:10]
    assert (film[ok] > 0).any()


# ---------------------------------------------------------------------------------------------- 4. unbiased with bounces, MIS and guiding
BOX = 556.0
N_SEEDS = 8
NGON = 128
_ARMS = {}


def _box(own_light):
    """ppg_host.cbox_scene(64, 48) scaled to unit size (tests/test_delta_emitters_gpu.py _unit_cbox), with or without its own emitter"""
    import ppg_host
    d = ppg_host.cbox_scene(64, 48)
    d.positions = (np.asarray(d.positions, np.float64) / BOX).astype(f32)
    d.camera = ppg_host.scenes.perspective_camera((278 / BOX, 273 / BOX, -800 / BOX), (278 / BOX, 273 / BOX, -799 / BOX), (0, 1, 0), 39.3077, "smaller",
                                                  10.0 / BOX, 2800.0 / BOX, 64, 48)
    assert d.normals is None  # flat shading: the meshes appended below are flat-shaded too
    if not own_light:
        d.tri_emitter = np.full_like(np.asarray(d.tri_emitter), -1)
        d.emitters = []
    return d


def _append_mesh(d, verts, tris, material, emitter):
    base = len(d.positions)
    d.positions = np.concatenate([np.asarray(d.positions, f32), np.asarray(verts, f32)])
    d.indices = np.concatenate([np.asarray(d.indices, np.uint32), (np.asarray(tris) + base).astype(np.uint32)])
    d.tri_material = np.concatenate([np.asarray(d.tri_material, np.uint32), np.full(len(tris), material, np.uint32)])
    d.tri_emitter = np.concatenate([np.asarray(d.tri_emitter, np.int32), np.full(len(tris), emitter, np.int32)])


DISK_C, DISK_R = (0.5, 0.9, 0.5), 0.12          # under the ceiling, facing down
DISK_ROT = _rot((1, 0, 0), 90)                   # object z -> world -y
CYL_BASE, CYL_R, CYL_L = (0.25, 0.72, 0.45), 0.05, 0.5
CYL_ROT = _rot((0, 1, 0), 90)                    # object z -> world x: a horizontal tube


def _fan(center, radius, R):
    """a regular 128-gon of the disk's area, as a fan with the disk's orientation"""
    rp = math.sqrt(math.pi * radius ** 2 / (0.5 * NGON * math.sin(2 * math.pi / NGON)))
    a = 2 * math.pi * np.arange(NGON) / NGON
    v = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([rp * np.cos(a), rp * np.sin(a), np.zeros(NGON)], 1)]) @ R.T + np.asarray(center)
    return v, [(0, 1 + k, 1 + (k + 1) % NGON) for k in range(NGON)]


def _tube(base, R, radius, length):
    """a 128-sided prism of the cylinder's area, normals outward"""
    rp = math.pi * radius / (NGON * math.sin(math.pi / NGON))
    a = 2 * math.pi * np.arange(NGON) / NGON
    ring = np.stack([rp * np.cos(a), rp * np.sin(a), np.zeros(NGON)], 1)
    v = np.concatenate([ring, ring + (0, 0, length)]) @ R.T + np.asarray(base)
    tris = []
    for k in range(NGON):
        k1 = (k + 1) % NGON
        tris += [(k, k1, NGON + k1), (k, NGON + k1, NGON + k)]
    return v, tris


def _emitter_scene(which, analytic):
    d = _box(False)
    d.materials = list(d.materials) + [dict(type=0, reflectance=(0.0, 0.0, 0.0))]
    mat = len(d.materials) - 1
    d.emitters = [dict(radiance=(20.0, 18.0, 12.0))]
    if which == "disk":
        if analytic:
            d.shapes = [_disk(DISK_C, DISK_R, DISK_ROT, material=mat, emitter=0)]
        else:
            _append_mesh(d, *_fan(DISK_C, DISK_R, DISK_ROT), mat, 0)
    else:
        if analytic:
            d.shapes = [_cylinder(CYL_BASE, CYL_ROT, CYL_R, CYL_L, material=mat, emitter=0)]
        else:
            _append_mesh(d, *_tube(CYL_BASE, CYL_ROT, CYL_R, CYL_L), mat, 0)
    return d


def _reflector_scene(analytic):
    """a two-sided diffuse disk and cylinder under the box's own light"""
    d = _box(True)
    d.materials = list(d.materials) + [dict(type=0, reflectance=(0.7, 0.6, 0.3), twosided=True)]
    mat = len(d.materials) - 1
    c, rot = (0.3, 0.45, 0.35), _rot((1, 0, 0), 60)
    base, crot = (0.55, 0.25, 0.3), _rot((1, 0, 0), -70) @ _rot((0, 1, 0), 25)
    if analytic:
        d.shapes = [_disk(c, 0.15, rot, material=mat, emitter=-1), _cylinder(base, crot, 0.08, 0.4, material=mat, emitter=-1)]
    else:
        _append_mesh(d, *_fan(c, 0.15, rot), mat, -1)
        _append_mesh(d, *_tube(base, crot, 0.08, 0.4), mat, -1)
    return d


def _arm(name, desc, **extra):
    """films of N_SEEDS renders (127 samples, bounces, the IMPROVED preset) reduced to 8 x 6 block means; computed once per name"""
    import ppg_host
    if name not in _ARMS:
        out = []
        for seed in range(N_SEEDS):
            props = dict(budgetType="spp", budget=127, maxDepth=10, rrDepth=10, strictNormals=1, hideEmitters=1, nee="always", seed=100 + seed, **IMPROVED)
            props.update(extra)
            img = ppg_host.GuidedPathTracer(engine=hip(**props)).render(desc).astype(np.float64).mean(2)
            out.append(img.reshape(6, 8, 8, 8).mean((1, 3)))
        _ARMS[name] = np.stack(out)
        assert np.isfinite(_ARMS[name]).all() and _ARMS[name].mean() > 0
    return _ARMS[name]


def _compare(name, x, y):
    """|mean1 - mean2| <= 4 sqrt(se1^2 + se2^2) for the whole image and for all but at most two of the 48 blocks; the standard errors must be
    small enough to see a 20 % error (tests/test_delta_emitters_gpu.py _compare)"""
    def stats(v):
        return v.mean(0), v.std(0, ddof=1) / math.sqrt(len(v))
    (mx, sx), (my, sy) = stats(x.mean((1, 2))), stats(y.mean((1, 2)))
    bound = 4 * math.hypot(sx, sy)
    print("%s: image means %.6g / %.6g, difference %.3g, bound %.3g (%.1f %% of the mean)" % (name, mx, my, abs(mx - my), bound, 100 * bound / mx))
    (bx, ex), (by, ey) = stats(x), stats(y)
    num, den = np.abs(bx - by), 4 * np.sqrt(ex ** 2 + ey ** 2)
    z = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))  # (a block that is black in every film of both arms agrees)
    print("%s: blocks over their bound: %d of 48 (largest ratio %.2f)" % (name, (z > 1).sum(), z.max()))
    assert bound < 0.2 * mx, "standard errors too large to see a 20 % error"
    assert abs(mx - my) <= bound
    assert (z > 1).sum() <= 2


def test_disk_emitter_matches_a_fan_of_equal_area():
    """(the 128-gon's residual bias — its silhouette against the circle's at equal area — is O((pi / 128)^2) = 6e-4, far below the bound)"""
    _compare("disk emitter vs 128-gon", _arm("disk", _emitter_scene("disk", True)), _arm("fan", _emitter_scene("disk", False)))


def test_cylinder_emitter_matches_a_tube_of_equal_area():
    _compare("cylinder emitter vs 128-sided tube", _arm("cylinder", _emitter_scene("cylinder", True)), _arm("tube", _emitter_scene("cylinder", False)))


def test_disk_emitter_with_and_without_next_event_estimation():
    """nee = never finds the disk by hitting it (Le on the hit side), nee = always samples it and weighs both by MIS with the hit-side pdfDirect"""
    _compare("nee always vs never", _arm("disk", _emitter_scene("disk", True)), _arm("disk never", _emitter_scene("disk", True), nee="never"))


def test_disk_emitter_guided_and_unguided():
    _compare("guided vs unguided", _arm("disk", _emitter_scene("disk", True)),
             _arm("disk unguided", _emitter_scene("disk", True), bsdfSamplingFraction=1.0, bsdfSamplingFractionLoss="none"))


def test_diffuse_disk_and_cylinder_match_their_meshes():
    _compare("reflectors vs meshes", _arm("reflectors", _reflector_scene(True)), _arm("reflector meshes", _reflector_scene(False)))


# ---------------------------------------------------------------------------------------------- 5. host paths
GUIDED = dict(budgetType="spp", budget=31, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=23)


def _lit_box(w=64, h=48):
    """the Cornell box with its own light, an emitting disk, an emitting flipped cylinder and a diffuse cylinder"""
    import ppg_host
    d = ppg_host.cbox_scene(w, h)
    d.materials = list(d.materials) + [dict(type=0, reflectance=(0.0, 0.0, 0.0)), dict(type=0, reflectance=(0.6, 0.6, 0.2), twosided=True)]
    black, yellow = len(d.materials) - 2, len(d.materials) - 1
    n0 = len(d.emitters)
    d.emitters = list(d.emitters) + [dict(radiance=(9.0, 6.0, 3.0)), dict(radiance=(2.0, 4.0, 8.0))]
    d.shapes = [_disk((150.0, 400.0, 200.0), 60.0, _rot((1, 0, 0), 70), material=black, emitter=n0),
                _cylinder((380.0, 300.0, 150.0), _rot((1, 0, 0), -60), 40.0, 150.0, flip=True, material=black, emitter=n0 + 1),
                _cylinder((250.0, 120.0, 100.0), _rot((0, 1, 0), 70), 30.0, 200.0, material=yellow, emitter=-1)]
    return d


def test_render_with_shapes_is_deterministic_and_an_empty_list_changes_nothing():
    import ppg_host
    props = dict(GUIDED, **IMPROVED)
    out = []
    for _ in range(2):
        gpt = ppg_host.GuidedPathTracer(engine=hip(**props))
        out.append((gpt.render(_lit_box()), gpt.engine.read_sdtree()))
    assert np.array_equal(out[0][0], out[1][0]) and np.isfinite(out[0][0]).all() and out[0][0].mean() > 0
    _tree_equal(out[0][1], out[1][1])
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 48))
    assert not np.array_equal(out[0][0], plain)
    # the same scene without ppg_set_shapes ever being called: the empty list set_scene sends changes nothing
    e = hip(**props)
    e.set_shapes = lambda shapes: None
    never = ppg_host.GuidedPathTracer(engine=e).render(ppg_host.cbox_scene(64, 48))
    assert np.array_equal(never, plain)


def test_a_shape_renders_the_same_bits_in_every_family_above_its_own():
    """The box with one emitting disk through the shapes kernels, then — an unused general microfacet entry — through the extended ones, then —
    an unused coated material on top — through the coat ones: each family holds the code of those below it, so film and SD-tree are equal."""
    import ppg_host
    from test_bsdfs import GOLD
    from test_coatings import DIFFUSE
    from test_coatings_gpu import UNUSED_COATED, _render, with_slices

    def box(extra):
        d = ppg_host.cbox_scene(16, 12)
        d.materials = list(d.materials) + [dict(type=0, reflectance=(0.0, 0.0, 0.0))]
        d.emitters = list(d.emitters) + [dict(radiance=(9.0, 6.0, 3.0))]
        d.shapes = [_disk((150.0, 400.0, 200.0), 60.0, _rot((1, 0, 0), 70), material=len(d.materials) - 1, emitter=len(d.emitters) - 1)]
        if extra:
            with_slices(d, extra)  # on no triangle and no shape: they only pick the family
        return d
    fa, ta = _render(box([]))
    fb, tb = _render(box([dict(GOLD, alpha_v=0.1), DIFFUSE]))
    fc, tc = _render(box([dict(GOLD, alpha_v=0.1), UNUSED_COATED]))
    assert np.isfinite(fa).all() and fa.mean() > 0
    assert np.array_equal(fa, fb) and np.array_equal(fa, fc)
    _tree_equal(ta, tb)
    _tree_equal(ta, tc)
    # (the disk is in the picture: without it the film differs)
    assert not np.array_equal(fa, _render(ppg_host.cbox_scene(16, 12))[0])


def test_two_shards_in_one_process_equal_the_unsharded_film():
    """two contexts with shards 0 and 1 of 2, their buffers summed as a reducer would, against one context"""
    import torch
    import ppg_host
    from ppg_host.distributed import _view
    dev = torch.device("cuda", 0)
    w, h = 64, 48
    scene = _lit_box(w, h)
    props = dict(GUIDED, sppPerPass=1, budget=47)
    ref_gpt = ppg_host.GuidedPathTracer(engine=hip(**props))
    ref_img = ref_gpt.render(scene)
    schedule = [it["passes"] for it in ref_gpt.iterations]
    assert schedule == [1, 2, 4, 8, 32]

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


def test_cpp_driver_equals_python_on_a_scene_with_shapes(tmp_path):
    import ppg_host
    from test_cpp_host import read_pfm
    exe = os.path.join(ROOT, "practical-path-guiding_amd", "bin", "ppg_render")
    path = str(tmp_path / "cbox-shapes.ppgs")
    ppg_host.save_scene(_lit_box(), path)
    props = dict(budgetType="spp", budget=28, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=4, **{k: v for k, v in IMPROVED.items() if k != "sppPerPass"})
    out = str(tmp_path / "out.pfm")
    args = [exe, "-q", "-o", out] + sum([["-D", "%s=%s" % kv] for kv in props.items()], [])
    r = subprocess.run(args + [path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    back = ppg_host.load_scene_file(path)
    assert len(back.shapes) == 3
    img = ppg_host.GuidedPathTracer(engine=hip(**props)).render(back)
    assert np.array_equal(read_pfm(out), img) and img.mean() > 0
    bare = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 48))
    assert not np.array_equal(img, bare)


def _tree_box(desc):
    e = hip(budgetType="spp", budget=4, nee="always")
    e.set_scene(desc)
    e.render()
    t = e.read_sdtree()
    e.close()
    return t["aabb_min"].astype(np.float64), t["aabb_max"].astype(np.float64)


def _enlarged(mn, mx):
    """the kd-tree's box around the geometry: enlarged by 1e-3 of its extent + 1e-3 (ppg_set_scene "Scene::getAABB")"""
    lo = mn - ((mx - mn) * 1e-3 + 1e-3)
    return lo, mx + ((mx - lo) * 1e-3 + 1e-3)


def test_the_scene_box_takes_in_a_far_disk_and_a_far_cylinder():
    base = _scene(False)
    base.shapes = []
    lo0, hi0 = _tree_box(base)
    # a disk far out along -x / +y: the box of its four extreme points (+-1, 0, 0), (0, +-1, 0) transformed
    R, c, rad = _rot((1, 2, 0.5), 40), np.array([-20.0, 15.0, 1.0]), 2.0
    d = _scene(False)
    d.shapes = [_disk(c, rad, R, material=1, emitter=-1)]
    m = np.asarray(d.shapes[0]["to_world"], np.float64).reshape(3, 4)
    pts = np.array([m[:, 3] + sg * m[:, k] for k in (0, 1) for sg in (1, -1)])
    want_lo, want_hi = _enlarged(np.minimum(pts.min(0), (-3, -3, QUAD_Z)), np.maximum(pts.max(0), (3, 3, QUAD_Z)))
    lo, hi = _tree_box(d)
    want_lo, want_hi = np.minimum(want_lo, CAM_O), np.maximum(want_hi, CAM_O)   # the sensor's position is part of the scene's box
    print("disk: box min %r (want %r), max %r (want >= %r)" % (lo, want_lo, hi, want_hi))
    assert np.allclose(lo, want_lo, rtol=1e-6, atol=1e-6) and (hi >= want_hi - 1e-5).all() and lo[0] < lo0[0] - 10 and hi[1] > hi0[1] + 5
    # (what is read back is the SD-tree's box: the scene's box made a cube from its min corner, as the reference's STree constructor does —
    # so the max corner is the getAABB value on the longest axis and min + that extent on the others)
    assert np.allclose(hi, want_lo + (want_hi - want_lo).max(), rtol=1e-6, atol=1e-5), (hi, want_lo + (want_hi - want_lo).max())
    # a cylinder far out along +z: the box of its two end circles, component-wise
    R, b_, rad, ln = _rot((0.2, 1, 0.3), 55), np.array([2.0, -1.0, 30.0]), 1.5, 6.0
    d = _scene(False)
    d.shapes = [_cylinder(b_, R, rad, ln, material=1, emitter=-1)]
    m = np.asarray(d.shapes[0]["to_world"], np.float64).reshape(3, 4)
    rng_ = rad * np.hypot(m[:, 0], m[:, 1])
    p0, p1 = m[:, 3], m[:, 3] + ln * m[:, 2]
    mn, mx = np.minimum(p0 - rng_, p1 - rng_), np.maximum(p0 + rng_, p1 + rng_)
    want_lo, want_hi = _enlarged(np.minimum(mn, (-3, -3, QUAD_Z)), np.maximum(mx, (3, 3, QUAD_Z)))
    want_lo, want_hi = np.minimum(want_lo, CAM_O), np.maximum(want_hi, CAM_O)
    lo, hi = _tree_box(d)
    print("cylinder: box min %r (want %r), max %r (want >= %r)" % (lo, want_lo, hi, want_hi))
    assert np.allclose(lo, want_lo, rtol=1e-6, atol=1e-6) and (hi >= want_hi - 1e-5).all() and hi[2] > hi0[2] + 20
    # (what is read back is the SD-tree's box: the scene's box made a cube from its min corner, as the reference's STree constructor does —
    # so the max corner is the getAABB value on the longest axis and min + that extent on the others)
    assert np.allclose(hi, want_lo + (want_hi - want_lo).max(), rtol=1e-6, atol=1e-5), (hi, want_lo + (want_hi - want_lo).max())


def test_cleared_list_renders_the_plain_scene_as_a_fresh_context_does():
    import ppg_host
    props = dict(budgetType="spp", budget=12, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=8)
    plain = ppg_host.cbox_scene(48, 40)
    fresh = hip(**props)
    fresh.set_scene(plain)
    fresh.render()
    want = fresh.read_film()
    e = hip(**props)
    e.set_scene(_lit_box(48, 40))
    e.render()
    lit = e.read_film()
    assert not np.array_equal(lit, want)
    e.set_shapes([])                  # ppg_set_shapes(ctx, NULL, 0), then ppg_set_scene with the plain scene
    e.set_scene(plain)
    e.render()
    assert np.array_equal(e.read_film(), want)
    e.set_scene(_lit_box(48, 40))     # and back, through the scene descriptions alone
    e.render()
    assert np.array_equal(e.read_film(), lit)
    e.close()


def test_set_scene_refuses_bad_shapes_and_the_call_is_refused_inside_a_render():
    import ppg_host
    from ppg_host.bindings import PPGError, Shape
    e = hip(budgetType="spp", budget=4, nee="always")
    good = _scene()
    disk, cyl = good.shapes[0], good.shapes[2]
    nan = float("nan")

    def with_matrix(rec, fn):
        m = np.asarray(rec["to_world"], np.float64).reshape(3, 4).copy()
        fn(m)
        return dict(rec, to_world=[float(v) for v in m.reshape(-1)])

    def shear(m): m[:, 1] += 0.3 * m[:, 0]
    def stretch(m): m[:, 1] *= 1.5
    def flatten(m): m[:, 2] = m[:, 0]
    def poison(m): m[1, 3] = nan
    unknown = Shape.from_dict(disk)
    unknown.type = 2
    textured = dict(type=0, reflectance=(0.5, 0.5, 0.5), texture=0)
    bad = [(unknown, "unknown type"), (with_matrix(disk, poison), "not finite"), (dict(cyl, radius=nan), "not finite"),
           (with_matrix(disk, shear), "shear"), (with_matrix(disk, stretch), "non-uniform scale"), (with_matrix(disk, flatten), "singular"),
           (dict(cyl, radius=0.0), "radius must be > 0"), (dict(cyl, length=-1.0), "length must be > 0"), (with_matrix(cyl, stretch), "not a rotation"),
           (with_matrix(cyl, shear), "not a rotation"), (dict(disk, material=99), "material index out of range"),
           (dict(cyl, emitter=0), "emitter is shared"), (dict(disk, material=3), "textured BSDFs are only supported on triangle meshes")]
    for rec, msg in bad:
        d = _scene()
        d.materials = list(d.materials) + [textured]
        d.textures = [dict(rgb=np.full((2, 2, 3), 0.5, f32))]
        d.texcoords = np.zeros((len(d.positions), 2), f32)
        if isinstance(rec, dict) and msg != "emitter is shared":
            rec = dict(rec, emitter=1)       # (shape 0 keeps emitter 0: only the one case shares it)
        d.shapes = [d.shapes[0], rec]
        with pytest.raises(PPGError, match=msg) as ex:
            e.set_scene(d)
        assert ex.value.code == -1 and "shape 1" in str(ex.value), str(ex.value)
    # an emitter id shared with a triangle, and a specular / alpha / opacity bitmap on a shape's material
    d = _scene()
    d.tri_emitter = np.array([2, -1], np.int32)
    with pytest.raises(PPGError, match="emitter is shared") as ex:
        e.set_scene(d)
    assert "shape 2" in str(ex.value)
    d = _scene()
    d.materials = list(d.materials) + [dict(type=5, reflectance=(0.5, 0.5, 0.5), specular=(1.0, 1.0, 1.0), eta=(1.5, 1.5, 1.5), specular_texture=0)]  # (plastic)
    d.textures = [dict(rgb=np.full((2, 2, 3), 0.5, f32))]
    d.texcoords = np.zeros((len(d.positions), 2), f32)
    d.shapes[3] = dict(d.shapes[3], material=3)
    with pytest.raises(PPGError, match="texture slot") as ex:
        e.set_scene(d)
    assert ex.value.code == -1 and "shape 3" in str(ex.value)
    # the call is refused while a render is open
    e.set_scene(good)
    e.begin_render()
    with pytest.raises(PPGError, match="ppg_begin_render") as ex:
        e.set_shapes([])
    assert ex.value.code == -3
    e.end_render()
    e.set_shapes([])
    e.close()
