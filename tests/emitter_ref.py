"""Emitter sampling and its MIS density restated in float64 from the reference's text: the emitter choice with sample re-use (scene.cpp:876-897,
pmf.h), AreaLight::sampleDirect / pdfDirect on a triangle mesh (area.cpp:158-183, shape.cpp:97-126, triangle.cpp:24-58, warp.cpp), Sphere::
sampleDirect / pdfDirect (sphere.cpp:291-378), the constant environment (constant.cpp:176-254) and the environment map (envmap.cpp:255-322,
381-407, 510-633, 657-662).  Plain numpy, no code of the project.

What is discrete is float32, what is continuous is float64.  The tables — the selection cdf, the area cdfs, the envmap's row and column cdfs —
are float32 running sums built as SceneBuilder::emitterTables / ::envmap (csrc/ppg_scene_build.h) and the oracle build them, the binary
searches run on them with the float32 sample, and the re-used sample (v - cdf[i]) / (cdf[i + 1] - cdf[i]) is the float32 quotient, because
the next choice is made with it.  Every choice of an interval therefore is the device's bit for bit and only the arithmetic behind the
choices is in double.  The envmap's row weights are sin((y + 0.5) pi / h) of the shared float math (include/ppg_detmath.h ppg_sincos): the
caller hands that function in (`sincos32`), since a float32 table cannot be restated from another sine.

Bounds.  B = 2e-5 as in tests/test_analytic_shapes_gpu.py: a device result is the end of about 40 rounded float32 operations, 40 x 6e-8 =
2.4e-6 relative, and the bound is ten times that; positions carry `scale` = the size of the numbers involved.  B is multiplied by the
conditioning of each result:
  1 / |dot(d, n)|       a density in solid angle and a root of a ray against a sphere
  scale / dist          a direction normalised from the difference of two points
  0.075 / s             a sine (or cosine) s = sqrt(1 - c^2) of a c close to 1: c^2 and c carry 5 ulp(1) = 3e-7 together, ten times that is
                        0.15 B, and d sqrt(x) = dx / (2 s).  It bounds the direction inside the sphere's cone, whose sines are at most
                        sinAlpha, and the cosine-weighted and uniform directions of the constant environment.
  (baseT - projDist)^2 / (r |dot(d, n)|)   the root of Sphere::sampleDirect's quadratic, see _sphere
  1 / (1 - cosAlpha)    the cone's density 1 / (2 pi (1 - cosAlpha)): cosAlpha carries about 2 ulp(1)
  0.16 / sinTheta       the envmap's density divided by sin(theta): theta = pixelSize (posY + 0.5) carries two roundings of up to half an
                        ulp(pi) = 1.2e-7 each and ppg_sincos 7.8e-8 absolute, together 3.2e-7 = 0.016 B; ten times that
Bilinear envmap lookups: the restatement is evaluated at the lookup position and at the four positions shifted by +- the float32 rounding
of the position, and the spread is added to B times the value (lookup_spread).  A bilinear lookup and the density built on it are
continuous across texel lines, so no item needs to be left out there; what is left out of the continuous comparisons is named in `skip`:
|dot(d, n)| or |dot(d, refN)| below 1e-4, the sphere's switch at sinAlpha = 1 - 1e-4 within rounding, and a bounding-sphere test within
rounding.  The discrete outputs of such items still count."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
B = 2e-5
EPS = 1e-4  # PPG_EPSILON
INV_PI = 1.0 / math.pi
MARGIN = 1e-4
LUM = (f32(0.212671), f32(0.715160), f32(0.072169))


# ------------------------------------------------------------------------------------------------------------ float32 tables and choices
def f32_cdf(values):
    """DiscreteDistribution: float32 running sums, then normalize() (pmf.h:101-114) -> (cdf [n + 1], sum, normalization)"""
    cdf = np.zeros(len(values) + 1, f32)
    for i, v in enumerate(values):
        cdf[i + 1] = f32(cdf[i] + f32(v))
    total = f32(cdf[-1])
    norm = f32(0)
    if total > 0:
        norm = f32(f32(1) / total)
        cdf[1:] = (cdf[1:] * norm).astype(f32)
        cdf[-1] = f32(1)
    return cdf, total, norm


def pmf_sample(cdf, v):
    """DiscreteDistribution::sample (pmf.h:124-136): lower_bound, clamp, then forward over intervals of width 0"""
    v = np.asarray(v, f32)
    n = len(cdf)
    idx = np.clip(np.searchsorted(cdf, v, side="left").astype(np.int64) - 1, 0, n - 2)
    for _ in range(n):
        step = (idx < n - 1) & (cdf[np.minimum(idx + 1, n - 1)] - cdf[idx] == 0)
        if not step.any():
            break
        idx = idx + step
    return idx


def reuse(cdf, idx, v):
    """sampleReuse (pmf.h:183-188): the float32 quotient, as the next choice is made with it"""
    with np.errstate(all="ignore"):
        return ((np.asarray(v, f32) - cdf[idx]).astype(f32) / (cdf[idx + 1] - cdf[idx]).astype(f32)).astype(f32)


def envmap_index(cdf, size, v):
    """sampleReuse of envmap.cpp:657-662: lower_bound over size + 1 entries, clamped; no forward skip"""
    return np.clip(np.searchsorted(cdf[:size + 1], np.asarray(v, f32), side="left").astype(np.int64) - 1, 0, size - 1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return (a * b).sum(-1)


def _tent(s):
    """warp::intervalToTent (warp.cpp:143-155)"""
    lo = s < 0.5
    t = np.where(lo, 2 * s, 2 * (s - 0.5))
    return np.where(lo, 1.0, -1.0) * (1 - np.sqrt(t))


def _concentric(sx, sy):
    """warp::squareToUniformDiskConcentric (warp.cpp:88-120)"""
    r1, r2 = 2 * sx - 1, 2 * sy - 1
    with np.errstate(all="ignore"):
        a = r1 * r1 > r2 * r2
        r = np.where(a, r1, r2)
        phi = np.where(a, (math.pi / 4) * (r2 / r1), (math.pi / 2) - (r1 / r2) * (math.pi / 4))
    zero = (r1 == 0) & (r2 == 0)
    r, phi = np.where(zero, 0.0, r), np.where(zero, 0.0, phi)
    return r * np.cos(phi), r * np.sin(phi)


def _frame(a):
    """coordinateSystem (util.cpp:592-601): (s, t) of Frame(a); the branch is taken on the float32 components"""
    big = np.abs(a[:, 0]) > np.abs(a[:, 1])
    with np.errstate(all="ignore"):
        il1 = 1 / np.sqrt(a[:, 0] ** 2 + a[:, 2] ** 2)
        il2 = 1 / np.sqrt(a[:, 1] ** 2 + a[:, 2] ** 2)
    z = np.zeros(len(a))
    with np.errstate(all="ignore"):
        t = np.where(big[:, None], np.stack([a[:, 2] * il1, z, -a[:, 0] * il1], 1), np.stack([z, a[:, 2] * il2, -a[:, 1] * il2], 1))
    return np.cross(t, a), t


def _uniform_sphere(sx, sy):
    """warp::squareToUniformSphere (warp.cpp:25-31) -> direction, r = sqrt(1 - z^2)"""
    z = 1 - 2 * sy
    r = np.sqrt(np.maximum(0.0, 1 - z * z))
    phi = 2 * math.pi * sx
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1), r


class EnvMapRef:
    """EnvironmentMap: tables in float32 (configure, envmap.cpp:255-322), lookups in float64"""

    def __init__(self, rgb, scale, to_world, sincos32):
        rgb = np.asarray(rgb, f32)
        self.h, self.w = rgb.shape[:2]
        h, w = self.h, self.w
        self.tex = rgb.astype(f64)
        self.scale = float(f32(scale))
        self.R = np.asarray(to_world, f32).reshape(3, 3).astype(f64)
        lum = ((rgb[..., 0] * LUM[0]).astype(f32) + (rgb[..., 1] * LUM[1]).astype(f32)).astype(f32)
        lum = (lum + (rgb[..., 2] * LUM[2]).astype(f32)).astype(f32)
        self.cols = np.zeros((h, w + 1), f32)
        self.rows = np.zeros(h + 1, f32)
        ang = ((np.arange(h, dtype=f32) + f32(0.5)).astype(f32) * f32(math.pi)).astype(f32) / f32(h)
        self.row_w32 = np.asarray(sincos32(ang.astype(f32)), f32)
        row_sum = f32(0)
        with np.errstate(all="ignore"):
            for y in range(h):
                c = f32(0)
                for x in range(w):
                    c = f32(c + lum[y, x])
                    self.cols[y, x + 1] = c
                norm = f32(f32(1) / c)
                self.cols[y, 1:] = (self.cols[y, 1:] * norm).astype(f32)
                self.cols[y, w] = f32(1)
                row_sum = f32(row_sum + f32(c * self.row_w32[y]))
                self.rows[y + 1] = row_sum
            norm = f32(f32(1) / row_sum)
            self.rows[1:] = (self.rows[1:] * norm).astype(f32)
            self.rows[h] = f32(1)
        self.row_w = self.row_w32.astype(f64)
        self.norm = 1.0 / (float(row_sum) * (2 * math.pi / w) * (math.pi / h))
        self.px, self.py = 2 * math.pi / w, math.pi / h

    def texel(self, x, y):
        return self.tex[np.clip(y, 0, self.h - 1), np.mod(x, self.w)]

    def lookup(self, pos_x, pos_y):
        """the bilinear lookup at (pos_x, pos_y) in texel units: value (rgb, before `scale`) and the density's numerator
        (lum(value1) rowWeight[yPos] + lum(value2) rowWeight[yPos + 1]) * normalization (envmap.cpp:575-588, 612-630)"""
        pos_x, pos_y = np.nan_to_num(pos_x), np.nan_to_num(pos_y)
        xp, yp = np.floor(pos_x).astype(np.int64), np.floor(pos_y).astype(np.int64)
        dx1, dy1 = pos_x - xp, pos_y - yp
        dx2, dy2 = 1 - dx1, 1 - dy1
        v1 = self.texel(xp, yp) * (dx2 * dy2)[:, None] + self.texel(xp + 1, yp) * (dx1 * dy2)[:, None]
        v2 = self.texel(xp, yp + 1) * (dx2 * dy1)[:, None] + self.texel(xp + 1, yp + 1) * (dx1 * dy1)[:, None]
        lum = lambda v: v @ np.array([float(LUM[0]), float(LUM[1]), float(LUM[2])])
        num = (lum(v1) * self.row_w[np.clip(yp, 0, self.h - 1)] + lum(v2) * self.row_w[np.clip(yp + 1, 0, self.h - 1)]) * self.norm
        return v1 + v2, num

    def lookup_spread(self, pos_x, pos_y, dx, dy):
        """the lookup, and how far it moves when the position moves by (+-dx, +-dy): the float32 rounding of the position"""
        v, num = self.lookup(pos_x, pos_y)
        sv, sn = np.zeros(len(pos_x)), np.zeros(len(pos_x))
        for ax, ay in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            v2, n2 = self.lookup(pos_x + ax * dx, pos_y + ay * dy)
            sv, sn = np.maximum(sv, np.abs(v2 - v).max(1)), np.maximum(sn, np.abs(n2 - num))
        return v, num, sv, sn

    def sample_direction(self, sx, sy):
        """internalSampleDirection (envmap.cpp:557-595) for float32 samples; a chosen interval of width 0 is a failed sample"""
        sx, sy = np.asarray(sx, f32), np.asarray(sy, f32)
        n = len(sx)
        row = envmap_index(self.rows, self.h, sy)
        fail = self.rows[row + 1] - self.rows[row] == 0
        sy2 = reuse(self.rows, row, sy)
        col = np.zeros(n, np.int64)
        sx2 = np.zeros(n, f32)
        col_w = np.zeros(n, f32)
        for r in np.unique(row[~fail]):
            m = (row == r) & ~fail
            col[m] = envmap_index(self.cols[r], self.w, sx[m])
            sx2[m] = reuse(self.cols[r], col[m], sx[m])
            col_w[m] = self.cols[r][col[m] + 1] - self.cols[r][col[m]]
        fail = fail | (col_w == 0)
        tx, ty = _tent(np.where(fail, 0.25, sx2.astype(f64))), _tent(np.where(fail, 0.25, sy2.astype(f64)))
        pos_x, pos_y = col + tx, row + ty
        v, num, sv, sn = self.lookup_spread(pos_x, pos_y, 2 * 6e-8 * self.w + 6e-8, 2 * 6e-8 * self.h + 6e-8)
        theta, phi = self.py * (pos_y + 0.5), self.px * (pos_x + 0.5)
        st, ct = np.sin(theta), np.cos(theta)
        d = np.stack([np.sin(phi) * st, ct, -np.cos(phi) * st], 1)
        den = np.maximum(np.abs(st), EPS)
        pdf = num / den
        out = dict(d=d, value=v * self.scale, pdf=pdf, fail=fail, row=row, col=col, row_w=(self.rows[row + 1] - self.rows[row]).astype(f64),
                   col_w=col_w.astype(f64), pos_x=pos_x, pos_y=pos_y, sin_theta=den, pole_cross=(pos_y + 0.5 <= 0) | (pos_y + 0.5 >= self.h),
                   wraps_x=(pos_x < 0) | (pos_x > self.w - 1), beyond_y=(pos_y < 0) | (pos_y > self.h - 1),
                   x_below=pos_x < 0, x_above=pos_x > self.w - 1, y_below=pos_y < 0, y_above=pos_y > self.h - 1)
        rel = B * (1 + 0.16 / den)
        out["tol_value"] = (sv + B * np.abs(v).max(1)) * self.scale
        out["tol_pdf"] = sn / den + pdf * rel
        for k in ("d", "value"):
            out[k] = np.where(fail[:, None], 0.0, out[k])
        out["pdf"] = np.where(fail, 0.0, out["pdf"])
        return out

    def _uv(self, d_local):
        d = d_local
        u = np.arctan2(d[:, 0], -d[:, 2]) * (INV_PI * 0.5) * self.w - 0.5
        v = np.arccos(np.clip(d[:, 1], -1, 1)) * INV_PI * self.h - 0.5
        # the float32 rounding of the position: the stated errors of dm_atan2 (2.29 ulp of up to pi) and dm_acos (3.73 ulp) through
        # 1 / 2 pi and 1 / pi and the size of the map, the products' own roundings, and one ulp of u * w
        du = self.w * (2.29 * 2.4e-7 / (2 * math.pi) + 3 * 6e-8) + 6e-8 * self.w
        dv = self.h * (3.73 * 2.4e-7 / math.pi + 3 * 6e-8) + 6e-8 * self.h
        if not np.array_equal(self.R, np.eye(3)):  # the rotation into the emitter's frame rounds the direction: 3 ulp, and d phi = dx / sin(theta)
            st = np.sqrt(np.maximum(1e-60, 1 - np.clip(d[:, 1], -1, 1) ** 2))
            du = du + self.w / (2 * math.pi) * 3 * 6e-8 / st
            dv = dv + self.h / math.pi * 3 * 6e-8 / st
            du, dv = np.minimum(du, 4.0 * self.w), np.minimum(dv, 4.0 * self.h)  # (beyond that the spread covers the whole map)
        return u, v, du, dv

    def eval(self, d_world):
        """evalEnvironment (envmap.cpp:381-407) -> radiance, its tolerance"""
        d = np.asarray(d_world, f64) @ self.R  # world -> emitter frame: the transpose of a rotation
        u, v, du, dv = self._uv(d)
        val, _, sv, _ = self.lookup_spread(u, v, du, dv)
        return val * self.scale, (sv + B * np.abs(val).max(1)) * self.scale

    def pdf_direction(self, d_local):
        """internalPdfDirection (envmap.cpp:598-633) -> density, its tolerance"""
        d = np.asarray(d_local, f64)
        u, v, du, dv = self._uv(d)
        _, num, _, sn = self.lookup_spread(u, v, du, dv)
        s2 = np.maximum(0.0, 1 - d[:, 1] ** 2)
        st = np.sqrt(s2)
        den = np.maximum(st, EPS)
        pdf = num / den
        with np.errstate(all="ignore"):
            rel = B * (1 + np.where(st > EPS, 0.015 / np.maximum(s2, 1e-300), 0.0))  # sqrt(1 - y^2): y^2 carries an ulp of 1
        return pdf, sn / den + pdf * rel

    def to_world(self, d_local):
        return d_local @ self.R.T


class EmitterRef:
    """The emitters of a scene description (ppg_host.scenes.SceneDesc): area emitters on triangles (with the face or the interpolated
    normal) and on analytic spheres, and the constant or image-based environment emitter.  Disks, cylinders and delta emitters take part
    in the choice only (kind "other")."""

    def __init__(self, desc, sincos32=None):
        P = np.asarray(desc.positions, f32).reshape(-1, 3)
        I = np.asarray(desc.indices, np.int64).reshape(-1, 3)
        te = np.asarray(desc.tri_emitter, np.int64).reshape(-1)
        self.P, self.I, self.tri_emitter = P.astype(f64), I, te
        self.N = None if desc.normals is None else np.asarray(desc.normals, f32).reshape(-1, 3).astype(f64)
        self.radiance = [np.asarray(e["radiance"], f32).astype(f64) for e in desc.emitters]
        self.spheres = list(desc.spheres or [])
        n_area = len(desc.emitters)
        self.kind, self.tris, self.acdf, self.inv_area, self.sphere_of = [], [], [], [], {}
        for k, s in enumerate(self.spheres):
            if s.get("emitter", -1) >= 0:
                self.sphere_of[s["emitter"]] = k
        shape_emitters = {s["emitter"] for s in (getattr(desc, "shapes", None) or []) if s.get("emitter", -1) >= 0}
        for e in range(n_area):
            t = np.flatnonzero(te == e)
            self.tris.append(t)
            areas = []
            for k in t:  # Triangle::surfaceArea (triangle.cpp:61-67) in float32, operation by operation
                p0, p1, p2 = P[I[k, 0]], P[I[k, 1]], P[I[k, 2]]
                a, b = (p1 - p0).astype(f32), (p2 - p0).astype(f32)
                c = [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]
                areas.append(f32(f32(0.5) * np.sqrt(f32(f32(f32(c[0] * c[0]) + f32(c[1] * c[1])) + f32(c[2] * c[2])))))
            cdf, total, _ = f32_cdf(areas)
            self.acdf.append(cdf)
            with np.errstate(all="ignore"):
                self.inv_area.append(float(f32(f32(1) / total)) if len(t) else -1.0)
            self.kind.append("sphere" if e in self.sphere_of else "other" if e in shape_emitters else "mesh" if len(t) else "empty")
        self.n_area = n_area
        self.n_delta = len(getattr(desc, "delta_emitters", None) or [])
        self.env = None if desc.environment is None else np.asarray(desc.environment, f32).astype(f64)
        self.envmap = None
        if desc.envmap is not None:
            self.envmap = EnvMapRef(desc.envmap["rgb"], desc.envmap.get("scale", 1.0), desc.envmap.get("to_world", np.eye(3).reshape(-1)), sincos32)
        self.has_env = self.env is not None or self.envmap is not None
        self.n_sel = n_area + self.n_delta + (1 if self.has_env else 0)
        self.kind += ["other"] * self.n_delta + (["env"] if self.has_env else [])
        self.sel_cdf, _, self.sel_norm = f32_cdf([1.0] * self.n_sel)
        if self.has_env:
            self.bs_c, self.bs_r = self._bsphere(desc)

    def _bsphere(self, desc):
        """AABB::getBSphere (aabb.cpp:44-47) of Scene::getAABB(): the kd-tree's padded box (MTS_KD_AABB_EPSILON) and the sensor's position,
        radius x 1.5 (constant.cpp:67-78); float32 throughout, it is a table"""
        P = np.asarray(desc.positions, f32).reshape(-1, 3)[np.asarray(desc.indices, np.int64).reshape(-1)]
        lo, hi = P.min(0), P.max(0)
        for s in self.spheres:
            c, r = np.asarray(s["center"], f32), f32(s["radius"])
            lo, hi = np.minimum(lo, (c - r).astype(f32)), np.maximum(hi, (c + r).astype(f32))
        eps = f32(1e-3)
        lo2 = (lo - (((hi - lo).astype(f32) * eps).astype(f32) + eps).astype(f32)).astype(f32)
        hi2 = (hi + (((hi - lo2).astype(f32) * eps).astype(f32) + eps).astype(f32)).astype(f32)
        cam = np.asarray(desc.camera["camera_to_world"], f32).reshape(4, 4)[:3, 3]
        lo2, hi2 = np.minimum(lo2, cam), np.maximum(hi2, cam)
        c = ((hi2 + lo2).astype(f32) * f32(0.5)).astype(f32)
        dv = (c - hi2).astype(f32)
        r = np.sqrt(f32(f32(f32(dv[0] * dv[0]) + f32(dv[1] * dv[1])) + f32(dv[2] * dv[2])))
        return c.astype(f64), float(max(f32(EPS), f32(f32(r) * f32(1.5))))

    # -------------------------------------------------------------------------------------------------------------------- the choice
    def choose(self, ux):
        """the emitter choice with sample re-use -> index, its probability (float32), the re-used sample (float32)"""
        ux = np.asarray(ux, f32)
        e = pmf_sample(self.sel_cdf, ux)
        em_pdf = (self.sel_cdf[e + 1] - self.sel_cdf[e]).astype(f32)
        return e, em_pdf, reuse(self.sel_cdf, e, ux)

    # ------------------------------------------------------------------------------------------------------------ one direct sample
    def sample_direct(self, ref, ref_n, u):
        ref32, rn32, u = np.asarray(ref, f32).reshape(-1, 3), np.asarray(ref_n, f32).reshape(-1, 3), np.asarray(u, f32).reshape(-1, 2)
        n = len(u)
        ref, rn = ref32.astype(f64), rn32.astype(f64)
        e, em_pdf, sx = self.choose(u[:, 0])
        out = dict(emitter=e, em_pdf=em_pdf, sx=sx, kind=np.array([self.kind[k] for k in e]), is_env=np.zeros(n, bool),
                   d=np.zeros((n, 3)), n=np.zeros((n, 3)), sd=np.zeros((n, 3)), value=np.zeros((n, 3)), dist=np.zeros(n), sdist=np.zeros(n), pdf=np.zeros(n),
                   lit=np.zeros(n, bool), skip=np.zeros(n, bool), sampled=np.zeros(n, bool), cond=np.ones(n),
                   tol_d=np.full(n, B), tol_n=np.full(n, B), tol_dist=np.full(n, B), tol_pdf=np.zeros(n), tol_value=np.zeros(n),
                   tol_sd=np.full(n, B), tol_sdist=np.full(n, B), extra={})
        for k in range(self.n_sel):
            m = e == k
            if not m.any():
                continue
            if self.kind[k] == "mesh":
                self._mesh(k, m, ref, rn, sx, u[:, 1], out)
            elif self.kind[k] == "sphere":
                self._sphere(k, m, ref, rn, sx, u[:, 1], out)
            elif self.kind[k] == "env":
                out["is_env"][m] = True
                (self._envmap if self.envmap is not None else self._const_env)(m, ref, rn, sx, u[:, 1], out)
        return out

    def _finish_area(self, k, m, ref, rn, p, nrm, out, tol_p, tol_n, extra_rel=0.0):
        """Shape::sampleDirect's conversion to solid angle (shape.cpp:102-115) and AreaLight::sampleDirect's facing tests (area.cpp:158-173)"""
        dv = p - ref[m]
        dist = np.linalg.norm(dv, axis=1)
        with np.errstate(all="ignore"):
            d = dv / dist[:, None]
            dn, dr = _dot(d, nrm), _dot(d, rn[m])
            pdf = np.where(dn != 0, self._area_pdf(k, ref[m], d, nrm, dist), 0.0)
            lit = (dr >= 0) & (dn < 0) & (pdf != 0)
            scale = 1 + np.abs(ref[m]).max(1) + np.abs(p).max(1)
            has_rn = (rn[m] != 0).any(1)
            out["skip"][m] |= (np.abs(dn) < MARGIN) | (has_rn & (np.abs(dr) < MARGIN)) | ~np.isfinite(pdf)
            cond = 1 / np.maximum(np.abs(dn), 1e-300)
            tol_pdf = pdf * (B * (2 + scale / dist + cond) + 2 * tol_p / dist + tol_n * cond + extra_rel)
            value = self.radiance[k][None, :] / pdf[:, None]
        out["sampled"][m] = True
        out["d"][m], out["dist"][m], out["n"][m], out["sd"][m], out["sdist"][m] = d, dist, nrm, d, dist
        out["tol_d"][m], out["tol_dist"][m], out["tol_n"][m] = (B * scale + tol_p) / dist, B * scale + tol_p, tol_n
        out["tol_sd"][m], out["tol_sdist"][m] = out["tol_d"][m], out["tol_dist"][m]
        out["cond"][m] = cond
        out["lit"][m] = lit
        out["pdf"][m] = np.where(lit, pdf, 0.0)
        out["value"][m] = np.where(lit[:, None], value, 0.0)
        out["tol_pdf"][m] = np.where(lit, tol_pdf, 0.0)
        with np.errstate(all="ignore"):
            out["tol_value"][m] = np.where(lit, value.max(1) * tol_pdf / pdf, 0.0)

    def _area_pdf(self, k, ref, d, nrm, dist):
        if self.kind[k] == "sphere":
            return self.sphere_pdf_direct(self.spheres[self.sphere_of[k]], ref, d, nrm, dist)[0]
        return self.inv_area[k] * dist ** 2 / np.abs(_dot(d, nrm))

    def _mesh(self, k, m, ref, rn, sx, uy, out):
        acdf, tris = self.acdf[k], self.tris[k]
        ti = pmf_sample(acdf, uy[m])
        sy = reuse(acdf, ti, uy[m]).astype(f64)
        s = sx[m].astype(f64)
        a = np.sqrt(np.maximum(0.0, 1 - s))  # warp::squareToUniformTriangle (warp.cpp:76-79)
        bx, by = 1 - a, a * sy
        I = self.I[tris[ti]]
        p0, p1, p2 = self.P[I[:, 0]], self.P[I[:, 1]], self.P[I[:, 2]]
        p = p0 + (p1 - p0) * bx[:, None] + (p2 - p0) * by[:, None]
        tol_n = np.full(len(s), B)
        with np.errstate(all="ignore"):
            if self.N is not None:
                raw = self.N[I[:, 0]] * (1 - bx - by)[:, None] + self.N[I[:, 1]] * bx[:, None] + self.N[I[:, 2]] * by[:, None]
                tol_n = B / np.linalg.norm(raw, axis=1)
                nrm = _unit(raw)
            else:
                nrm = _unit(np.cross(p1 - p0, p2 - p0))
        out["extra"].setdefault("tri", np.full(len(out["pdf"]), -1))[m] = tris[ti]
        out["extra"].setdefault("area_width", np.zeros(len(out["pdf"])))[m] = (acdf[ti + 1] - acdf[ti]).astype(f64)
        out["extra"].setdefault("bary", np.zeros((len(out["pdf"]), 2)))[m] = np.stack([bx, by], 1)
        self._finish_area(k, m, ref, rn, p, nrm, out, 0.0, tol_n)

    def sphere_pdf_direct(self, sp, ref, d, nrm, dist):
        """Sphere::pdfDirect (sphere.cpp:357-378) -> density, 1 / (1 - cosAlpha) (1 on the inside branch), whether the switch is within rounding"""
        c, r = np.asarray(sp["center"], f32).astype(f64), float(f32(sp["radius"]))
        with np.errstate(all="ignore"):
            sin_a = r / np.linalg.norm(c - ref, axis=1)
            cone = sin_a < 1 - EPS
            cos_a = np.sqrt(np.maximum(0.0, 1 - sin_a ** 2))
            inv_area = 1 / (4 * math.pi * r * r)
            pdf = np.where(cone, (INV_PI * 0.5) / (1 - cos_a), inv_area * dist ** 2 / np.abs(_dot(d, nrm)))
            cond = np.where(cone, 1 / (1 - cos_a), 1.0)
        return pdf, cond, np.abs(sin_a - (1 - EPS)) < 1e-6, sin_a

    def _sphere(self, k, m, ref, rn, sx, uy, out):
        sp = self.spheres[self.sphere_of[k]]
        c, r = np.asarray(sp["center"], f32).astype(f64), float(f32(sp["radius"]))
        flip = -1.0 if sp.get("flip_normals") else 1.0
        rf = ref[m]
        s, t = sx[m].astype(f64), uy[m].astype(f64)
        to_c = c - rf
        with np.errstate(all="ignore"):
            ref_dist = np.linalg.norm(to_c, axis=1)
            sin_a = r / ref_dist
            cone = sin_a < 1 - EPS
            cos_a = np.sqrt(np.maximum(0.0, 1 - sin_a ** 2))
            # outside: warp::squareToUniformCone (warp.cpp:54-63) in Frame(refToCenter / |refToCenter|), then the ray against the sphere
            cos_t = (1 - s) + s * cos_a
            sin_t = np.sqrt(np.maximum(0.0, 1 - cos_t ** 2))
            phi = 2 * math.pi * t
            a = to_c / ref_dist[:, None]
            a32 = a.astype(f32).astype(f64)  # (the branch of coordinateSystem is taken on float32 components)
            big = np.abs(a32[:, 0]) > np.abs(a32[:, 1])
            tF = np.where(big[:, None], _unit(np.stack([a[:, 2], np.zeros(len(a)), -a[:, 0]], 1)), _unit(np.stack([np.zeros(len(a)), a[:, 2], -a[:, 1]], 1)))
            sF = np.cross(tF, a)
            d_c = sF * (np.cos(phi) * sin_t)[:, None] + tF * (np.sin(phi) * sin_t)[:, None] + a * cos_t[:, None]
            proj = _dot(to_c, d_c)
            disc = proj ** 2 - (ref_dist ** 2 - r * r)
            near = proj - np.sqrt(np.maximum(disc, 0.0))
            p_c = rf + d_c * near[:, None]
            n_c = _unit(p_c - c)
            # inside: uniform over the sphere (warp::squareToUniformSphere)
            dv, _ = _uniform_sphere(s, t)
            p_i = c + dv * r
        p = np.where(cone[:, None], c + n_c * r, p_i)
        nrm = np.where(cone[:, None], n_c, dv) * flip
        dn_c = np.abs(_dot(d_c, n_c))
        with np.errstate(all="ignore"):
            tol_d = np.where(cone, B * (1 + 0.075 / np.maximum(sin_t, 1e-300)), 0.0)
            scale = 1 + np.abs(rf).max(1) + np.abs(c).max() + r
            # the reference intersects from `query`, baseT = refDist^2 / projDist along the ray: its quadratic's discriminant is a difference
            # of numbers of size 4 (baseT - projDist)^2, which carry 5 ulp (ten times that: 0.15 B), and d sqrt(x) = dx / (2 sqrt(x)) with
            # sqrt(discriminant) = 2 r |dot(d, n)|.  Close to the sphere and near its silhouette baseT is large and this term decides.
            base_t = ref_dist ** 2 / proj
            tol_root = 0.15 * B * (base_t - proj) ** 2 / (r * np.maximum(dn_c, 1e-300))
            tol_p = np.where(cone, (B * scale + near * tol_d) / np.maximum(dn_c, 1e-300) + tol_root, B * scale)
            tol_n = tol_p / r + B
            extra_rel = np.where(cone, B / (1 - cos_a), 0.0)
        out["skip"][m] |= np.abs(sin_a - (1 - EPS)) < 1e-6
        out["skip"][m] |= cone & (disc <= 0)
        ex = out["extra"]
        ex.setdefault("sin_alpha", np.zeros(len(out["pdf"])))[m] = sin_a
        ex.setdefault("cone", np.zeros(len(out["pdf"]), bool))[m] = cone
        self._finish_area(k, m, ref, rn, p, nrm, out, tol_p, tol_n, extra_rel)
        # on the cone branch the record's d is the sampled direction, dist = baseT + nearT along it, and the density is the cone's whatever
        # the normal; the shadow ray goes to c + n r (scene.cpp:889-893)
        idx = np.flatnonzero(m)[cone]
        with np.errstate(all="ignore"):
            out["d"][idx], out["dist"][idx] = d_c[cone], near[cone]
            out["tol_d"][idx] = tol_d[cone]
            dr, dn = _dot(d_c[cone], rn[m][cone]), _dot(d_c[cone], nrm[cone])
            pdf = (INV_PI * 0.5) / (1 - cos_a[cone])
            lit = (dr >= 0) & (dn < 0) & (pdf != 0)
            has_rn = (rn[m][cone] != 0).any(1)
            skip = (np.abs(dn) < MARGIN) | (has_rn & (np.abs(dr) < MARGIN)) | (np.abs(sin_a[cone] - (1 - EPS)) < 1e-6) | (disc[cone] <= 0)
            out["skip"][idx] = skip
            out["lit"][idx] = lit
            out["pdf"][idx] = np.where(lit, pdf, 0.0)
            val = self.radiance[k][None, :] / pdf[:, None]
            out["value"][idx] = np.where(lit[:, None], val, 0.0)
            tol_pdf = pdf * (2 * B + extra_rel[cone])
            out["tol_pdf"][idx] = np.where(lit, tol_pdf, 0.0)
            out["tol_value"][idx] = np.where(lit, val.max(1) * tol_pdf / pdf, 0.0)
            out["cond"][idx] = 1 / (1 - cos_a[cone])

    def _bsphere_hit(self, ref, d):
        """BSphere::rayIntersect (bsphere.h:88-95) -> hit, near, far, whether the tests on them are within rounding"""
        o = ref - self.bs_c
        A, Bq, C = _dot(d, d), 2 * _dot(o, d), _dot(o, o) - self.bs_r ** 2
        disc = Bq * Bq - 4 * A * C
        with np.errstate(all="ignore"):
            sq = np.sqrt(np.maximum(disc, 0.0))
            temp = np.where(Bq < 0, -0.5 * (Bq - sq), -0.5 * (Bq + sq))
            t0, t1 = temp / A, C / temp
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        scale = 1 + np.abs(ref).max(1) + np.abs(self.bs_c).max() + self.bs_r
        close = (np.abs(disc) < 8 * B * scale ** 2) | (np.abs(near) < 4 * B * scale) | (np.abs(far) < 4 * B * scale) | ~np.isfinite(near) | ~np.isfinite(far)
        return disc >= 0, near, far, close, scale

    def _env_point(self, m, ref, d, tol_d, out):
        """the point on the bounding sphere: p = ref + d farT, n towards the centre; the shadow ray from the end points"""
        hit, near, far, close, scale = self._bsphere_hit(ref[m], d)
        ok = hit & (near < 0) & (far > 0)
        p = ref[m] + d * far[:, None]
        with np.errstate(all="ignore"):
            nrm = _unit(self.bs_c - p)
            pd = p - ref[m]
            sdist = np.linalg.norm(pd, axis=1)
            sd = pd / sdist[:, None]
            cos_exit = np.abs(_dot(_unit(d), nrm))
            tol_dist = (B * scale + np.abs(far) * tol_d) / np.maximum(cos_exit, 1e-300)
        out["skip"][m] |= close
        out["sampled"][m] = ok
        for key, v in (("d", d), ("n", nrm), ("sd", sd)):
            out[key][m] = np.where(ok[:, None], v, 0.0)
        out["dist"][m], out["sdist"][m] = np.where(ok, far, 0.0), np.where(ok, sdist, 0.0)
        out["tol_d"][m], out["tol_dist"][m] = tol_d, tol_dist
        out["tol_n"][m] = (tol_dist + np.abs(far) * tol_d) / self.bs_r + B
        out["tol_sd"][m], out["tol_sdist"][m] = tol_d + B, tol_dist
        return ok

    def _const_env(self, m, ref, rn, sx, uy, out):
        s, t = sx[m].astype(f64), uy[m].astype(f64)
        a = rn[m]
        has_rn = (a != 0).any(1)
        px, py = _concentric(s, t)
        z = np.sqrt(np.maximum(0.0, 1 - px * px - py * py))
        z = np.where(z == 0, 1e-10, z)
        sF, tF = _frame(np.where(has_rn[:, None], a, [0.0, 0.0, 1.0]))
        d_h = sF * px[:, None] + tF * py[:, None] + a * z[:, None]
        d_u, r = _uniform_sphere(s, t)
        d = np.where(has_rn[:, None], d_h, d_u)
        pdf = np.where(has_rn, INV_PI * z, INV_PI * 0.25)
        with np.errstate(all="ignore"):
            tol_d = np.where(has_rn, B * (1 + 0.075 / z), B * (1 + 0.075 / np.maximum(r, 1e-300)))
            rel = np.where(has_rn, B * (1 + 0.075 / z ** 2), 1e-7)
        ok = self._env_point(m, ref, d, tol_d, out)
        dr = _dot(d, a)
        lit = ok & ~(has_rn & (dr <= 0))
        out["skip"][m] |= has_rn & (np.abs(dr) < MARGIN)
        out["lit"][m] = lit
        out["pdf"][m] = np.where(ok, pdf, 0.0)  # (the density stays where only the facing test fails: constant.cpp:207-213)
        out["value"][m] = np.where(lit[:, None], self.env[None, :] / pdf[:, None], 0.0)
        out["tol_pdf"][m] = pdf * rel
        out["tol_value"][m] = np.where(lit, self.env.max() / pdf * rel, 0.0)
        out["cond"][m] = np.where(has_rn, 1 / z ** 2, 1.0)
        out["extra"].setdefault("cos", np.zeros(len(out["pdf"])))[m] = np.where(has_rn, z, 1.0)

    def _envmap(self, m, ref, rn, sx, uy, out):
        E = self.envmap
        r = E.sample_direction(sx[m], uy[m])
        dw = E.to_world(r["d"])
        good = ~r["fail"] & (r["value"] != 0).any(1) & (r["pdf"] != 0)
        ok = self._env_point(m, ref, np.where(good[:, None], dw, [0.0, 1.0, 0.0]), np.full(len(dw), B), out) & good
        idx = np.flatnonzero(m)
        out["skip"][idx[~good]] = False  # (a failed sample has no bounding-sphere test)
        for key in ("d", "n", "sd"):
            out[key][idx[~ok]] = 0.0
        out["dist"][idx[~ok]], out["sdist"][idx[~ok]] = 0.0, 0.0
        out["sampled"][m] = ok
        out["lit"][m] = ok
        with np.errstate(all="ignore"):
            value = r["value"] / r["pdf"][:, None]
            tol_value = value.max(1) * (r["tol_value"] / np.abs(r["value"]).max(1) + r["tol_pdf"] / r["pdf"])
        out["pdf"][m] = np.where(ok, r["pdf"], 0.0)
        out["value"][m] = np.where(ok[:, None], value, 0.0)
        out["tol_pdf"][m] = np.where(ok, r["tol_pdf"], 0.0)
        out["tol_value"][m] = np.where(ok, tol_value, 0.0)
        out["cond"][m] = 1 / r["sin_theta"]
        n_all = len(out["pdf"])
        for key in ("row", "col", "pos_x", "pos_y", "pole_cross", "wraps_x", "beyond_y", "x_below", "x_above", "y_below", "y_above", "fail", "row_w", "col_w"):
            out["extra"].setdefault(key, np.zeros(n_all, r[key].dtype))[m] = r[key]

    # ------------------------------------------------------------------------------------------ the density of a BSDF-sampled ray
    def pdf_direct(self, rays, ref_n):
        """The emitter a ray finds and Scene::pdfEmitterDirect for it (scene.cpp:949-952), for scenes of a handful of triangles and
        spheres: every primitive is tested in double.  -> emitter, value, pdf_direct, emitter_pdf, tol (of pdf_direct), skip, hit"""
        rays, rn = np.asarray(rays, f32).reshape(-1, 8).astype(f64), np.asarray(ref_n, f32).reshape(-1, 3).astype(f64)
        o, d, mint, maxt = rays[:, :3], rays[:, 4:7], rays[:, 3], rays[:, 7]
        n = len(o)
        best, prim, edge = np.full(n, np.inf), np.full(n, -1), np.zeros(n, bool)
        with np.errstate(all="ignore"):
            for k, tri in enumerate(self.I):
                p0, p1, p2 = self.P[tri[0]], self.P[tri[1]], self.P[tri[2]]
                e1, e2 = p1 - p0, p2 - p0
                pv = np.cross(d, e2)
                det = pv @ e1
                tv = o - p0
                uu = _dot(tv, pv) / det
                qv = np.cross(tv, e1)
                vv = _dot(d, qv) / det
                t = qv @ e2 / det
                inside = (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t >= mint) & (t <= maxt) & (det != 0)
                near_edge = (np.minimum(np.minimum(uu, vv), 1 - uu - vv) > -MARGIN) & (np.minimum(np.minimum(uu, vv), 1 - uu - vv) < MARGIN) & (t > 0)
                edge |= near_edge & (t < best + MARGIN)
                take = inside & (t < best)
                best, prim = np.where(take, t, best), np.where(take, k, prim)
            for k, sp in enumerate(self.spheres):
                c, r = np.asarray(sp["center"], f32).astype(f64), float(f32(sp["radius"]))
                oc = o - c
                A, Bq, C = _dot(d, d), 2 * _dot(oc, d), _dot(oc, oc) - r * r
                disc = Bq * Bq - 4 * A * C
                sq = np.sqrt(np.maximum(disc, 0.0))
                t0, t1 = (-Bq - sq) / (2 * A), (-Bq + sq) / (2 * A)
                t = np.where(t0 >= mint, t0, t1)
                valid = (disc >= 0) & (t >= mint) & (t <= maxt) & ~((t0 < mint) & (t1 > maxt))
                edge |= (np.abs(disc) < 8 * MARGIN * r * r * A) | (valid & (np.abs(t - mint) < MARGIN * r))   # (disc = 4 A (r^2 - b^2), b the ray's distance from the centre)
                take = valid & (t < best)
                best, prim = np.where(take, t, best), np.where(take, len(self.I) + k, prim)
        out = dict(hit=prim >= 0, prim=prim, t=best, emitter=np.full(n, -1), value=np.zeros((n, 3)), pdf_direct=np.zeros(n), tol=np.zeros(n), skip=edge.copy(),
                   extra={})
        has_rn = (rn != 0).any(1)
        dr = _dot(d, rn)
        refn_ok = dr >= 0
        out["skip"] |= has_rn & (np.abs(dr) < MARGIN)
        n_tri = len(self.I)
        with np.errstate(all="ignore"):
            for k in np.unique(prim[prim >= 0]):
                m = prim == k
                if k < n_tri:
                    em = self.tri_emitter[k]
                    tri = self.I[k]
                    p0, p1, p2 = self.P[tri[0]], self.P[tri[1]], self.P[tri[2]]
                    p = o[m] + d[m] * best[m][:, None]
                    if self.N is not None:  # barycentric interpolation at the hit
                        e1, e2 = p1 - p0, p2 - p0
                        nn = np.cross(e1, e2)
                        bu = _dot(np.cross(p - p0, e2), nn) / (nn @ nn)
                        bv = _dot(np.cross(e1, p - p0), nn) / (nn @ nn)
                        nrm = _unit(self.N[tri[0]] * (1 - bu - bv)[:, None] + self.N[tri[1]] * bu[:, None] + self.N[tri[2]] * bv[:, None])
                    else:
                        nrm = np.broadcast_to(_unit(np.cross(p1 - p0, p2 - p0)), p.shape)
                else:
                    sp = self.spheres[k - n_tri]
                    em = sp.get("emitter", -1)
                    c = np.asarray(sp["center"], f32).astype(f64)
                    nrm = _unit(o[m] + d[m] * best[m][:, None] - c) * (-1.0 if sp.get("flip_normals") else 1.0)
                out["emitter"][m] = em
                if em < 0:
                    continue
                dn = _dot(d[m], nrm)
                seen = dn < 0  # AreaLight::eval (area.cpp:104-109): the emitter's front
                out["value"][m] = np.where(seen[:, None], self.radiance[em][None, :], 0.0)
                out["skip"][m] |= np.abs(dn) < MARGIN
                dist = best[m]
                scale = 1 + np.abs(o[m]).max(1) + dist
                cond = 1 / np.maximum(np.abs(dn), 1e-300)
                if self.kind[em] == "sphere":
                    pdf, c2, sw, _ = self.sphere_pdf_direct(self.spheres[self.sphere_of[em]], o[m], d[m], nrm, dist)
                    out["skip"][m] |= sw
                    rel = np.where(c2 > 1, B * (2 + c2), B * (2 + scale / dist + cond) * 2)
                else:
                    pdf = self.inv_area[em] * dist ** 2 / np.abs(dn)
                    rel = B * (2 + scale / dist + cond) * 2
                on = seen & refn_ok[m]
                out["pdf_direct"][m] = np.where(on, pdf, 0.0)
                out["tol"][m] = np.where(on, pdf * rel, 0.0)
            miss = prim < 0
            if self.has_env and miss.any():
                hit, near, far, close, _ = self._bsphere_hit(o[miss], d[miss])
                ok = hit & ~(near > 0) & ~(far < 0)
                idx = np.flatnonzero(miss)
                out["skip"][idx] |= close
                out["emitter"][idx[ok]] = self.n_sel - 1
                if self.envmap is not None:
                    val, _ = self.envmap.eval(d[idx])
                    pdf, tol = self.envmap.pdf_direction(d[idx] @ self.envmap.R)
                else:
                    val = np.broadcast_to(self.env, (len(idx), 3))
                    pdf = np.where(has_rn[idx], INV_PI * np.maximum(0.0, dr[idx]), INV_PI * 0.25)
                    tol = B * INV_PI * np.ones(len(idx))
                nz = ok & (val != 0).any(1)
                out["value"][idx] = np.where(ok[:, None], val, 0.0)
                out["pdf_direct"][idx] = np.where(nz, pdf, 0.0)
                out["tol"][idx] = np.where(nz, tol, 0.0)
        out["emitter_pdf"] = out["pdf_direct"] * float(self.sel_norm)
        return out


def triangle_quadrature(ref_pt, p0, p1, p2, radiance, n=400):
    """the integral of `radiance` over the solid angle a triangle (seen from its front, face normal) subtends at ref_pt: midpoint rule on
    n^2 sub-triangles of the barycentric grid"""
    e1, e2 = p1 - p0, p2 - p0
    nn = np.cross(e1, e2)
    area, nrm = 0.5 * np.linalg.norm(nn), nn / np.linalg.norm(nn)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    total = 0.0
    for up, (ci, cj) in ((True, (1 / 3, 1 / 3)), (False, (2 / 3, 2 / 3))):
        sel = (i + j < n) if up else (i + j < n - 1)
        b1, b2 = (i[sel] + ci) / n, (j[sel] + cj) / n
        p = p0 + e1 * b1[:, None] + e2 * b2[:, None]
        dv = p - ref_pt
        r2 = _dot(dv, dv)
        cos = -_dot(dv, nrm) / np.sqrt(r2)
        total += (np.maximum(cos, 0.0) / r2).sum() * area / n ** 2
    return np.asarray(radiance, f64) * total
