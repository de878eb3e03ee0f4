"""Mitsuba's `coating` and `roughcoating` adapters (include/ppg.h ppg_set_coatings), on the CPU:

  * a numpy restatement of both plug-ins and of the BSDFs they may wrap, in a precision of the caller's choice, written from the
    plug-ins' behaviour (a dielectric layer: refract in, query the nested BSDF, attenuate by the two transmittances and the absorption,
    compress the solid angle; the layer's own delta / glossy reflection as the last component) and checked on its own: a closed form,
    sample() against eval() and pdf(), a chi-square test of the sampled directions, the limits;
  * the same restatement run in float32 and in float64 over the lattice the GPU test (test_coatings_gpu.py) feeds the kernels: the
    figures that test derives its bounds from, and the share of items on which the two precisions take different branches;
  * the hosts: material dicts, both scene loaders, the flat scene file.
"""
import os
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import mitsuba_xml
from ppg_host.bindings import Coating

from test_bsdfs import GOLD, rtrans_slice, unit
from test_microfacet_general import WIS, Distribution

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LUM = (0.212671, 0.715160, 0.072169)

# the nested materials (tests/test_bsdfs.py's) and the two coat slices of tests/golden/rtrans_slices.npz
DIFFUSE = dict(type="diffuse", reflectance=(0.2, 0.5, 0.8))
COPPER = dict(type="conductor", eta=(0.200438, 0.924033, 1.102212), k=(3.912949, 2.452848, 2.142188), reflectance=(1, 1, 1))
PLASTIC = dict(type="plastic", reflectance=(0.6, 0.3, 0.1), specular=(1, 1, 1), eta=1.49)
ROUGHPLASTIC = dict(type="roughplastic", alpha=0.2, eta=1.49, distribution="beckmann", slice=rtrans_slice("beckmann", 0.2, 1.49),
                    reflectance=(0.2, 0.5, 0.7), specular=(0.8, 0.9, 1.0))
NESTED = dict(diffuse=DIFFUSE, gold=GOLD, copper=COPPER, plastic=PLASTIC, roughplastic=ROUGHPLASTIC)
SMOOTH_COAT = dict(kind="coating", eta=1.5, thickness=1.5, sigma_a=(0.4, 0.1, 0.02), specular=(0.9, 1.0, 0.8))
ROUGH_COATS = dict(ggx=dict(kind="roughcoating", eta=1.5, thickness=0.5, sigma_a=(0.1, 0.3, 0.6), specular=(1.0, 0.9, 0.8), alpha=0.1, distribution="ggx",
                            slice=rtrans_slice("ggx", 0.1, 1.5)),
                   beckmann=dict(kind="roughcoating", eta=1.49, thickness=1.0, sigma_a=(0, 0, 0), specular=(1, 1, 1), alpha=0.2, distribution="beckmann",
                                 slice=rtrans_slice("beckmann", 0.2, 1.49)))
# every allowed pairing: coating over the five leaves, roughcoating (both slices) over the three without a delta component
PAIRINGS = [("coating", n) for n in NESTED] + [("roughcoating-" + c, n) for c in ROUGH_COATS for n in ("diffuse", "gold", "roughplastic")]
CASES = [(c, n, ts) for c, n in PAIRINGS for ts in (False, True)]


def case_id(c):
    return "%s-%s%s" % (c[0], c[1], "-twosided" if c[2] else "")


def coat_of(name):
    return SMOOTH_COAT if name == "coating" else ROUGH_COATS[name.split("-")[1]]


# ------------------------------------------------------------------------------------------------ the restatement
def _v(a, dt):
    return np.asarray(a, dt).reshape(-1, 3)


def dot(a, b):
    return (a * b).sum(1)


def normalize(a):
    return a / np.sqrt(dot(a, a))[:, None]


def fresnel_dielectric(ci, eta, dt):
    """unpolarised Fresnel reflectance of a dielectric boundary with relative index eta, seen under cos theta = ci (from outside when
    ci > 0), and the cosine of the refracted direction (opposite sign; 0 and R = 1 on total internal reflection)"""
    ci = np.asarray(ci, dt)
    eta = dt(eta)
    with np.errstate(all="ignore"):
        scale = np.where(ci > 0, dt(1) / eta, eta)
        ct2 = dt(1) - (dt(1) - ci * ci) * (scale * scale)
        tir = ct2 <= 0
        a, ct = np.abs(ci), np.sqrt(np.maximum(ct2, dt(0)))
        rs = (a - eta * ct) / (a + eta * ct)
        rp = (eta * a - ct) / (eta * a + ct)
        r = dt(0.5) * (rs * rs + rp * rp)
    return np.where(tir, dt(1), r).astype(dt), np.where(tir, dt(0), np.where(ci > 0, -ct, ct)).astype(dt)


def fresnel_conductor(ci, eta, k, dt):
    """exact unpolarised reflectance of a conductor, per channel: [n, 3]"""
    ci = np.asarray(ci, dt)[:, None]
    eta, k = np.asarray(eta, dt)[None], np.asarray(k, dt)[None]
    c2 = ci * ci
    s2 = dt(1) - c2
    s4 = s2 * s2
    t1 = eta * eta - k * k - s2
    a2b2 = np.sqrt(np.maximum(t1 * t1 + k * k * eta * eta * dt(4), dt(0)))
    a = np.sqrt(np.maximum((a2b2 + t1) * dt(0.5), dt(0)))
    u1, u2 = a2b2 + c2, a * (dt(2) * ci)
    rs = (u1 - u2) / (u1 + u2)
    u3, u4 = a2b2 * c2 + s4, u2 * s2
    rp = rs * (u3 - u4) / (u3 + u4)
    return ((rp + rs) * dt(0.5)).astype(dt)


def diffuse_fresnel_reflectance(eta):
    """2 int_0^1 F(mu, eta) mu dmu = int_0^1 F(sqrt(t), eta) dt, by the rule the library states for it (include/ppg_detmath.h): Simpson's on
    4096 intervals of t.  (From inside, F has a square-root kink at the critical angle: a finer rule moves the value by 1e-5, which a
    comparison at float32 precision would see.)"""
    n = 4096
    f = fresnel_dielectric(np.sqrt(np.arange(n + 1) / n), eta, np.float64)[0]
    w = np.where(np.arange(n + 1) % 2 == 1, 4.0, 2.0)
    w[0] = w[-1] = 1.0
    return float((f * w).sum() / n / 3.0)


def cosine_hemisphere(u, dt):
    """Shirley and Chiu's concentric map of the square onto the disk, lifted to the hemisphere"""
    u = np.asarray(u, dt)
    r1, r2 = dt(2) * u[:, 0] - dt(1), dt(2) * u[:, 1] - dt(1)
    pi = dt(np.pi)
    with np.errstate(all="ignore"):
        first = r1 * r1 > r2 * r2
        r = np.where(first, r1, r2)
        phi = np.where(first, (pi / dt(4)) * (r2 / r1), (pi / dt(2)) - (r1 / r2) * (pi / dt(4)))
        phi = np.where((r1 == 0) & (r2 == 0), dt(0), phi)
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(np.maximum(dt(0), dt(1) - x * x - y * y))
    z = np.where(z == 0, dt(1e-10), z)
    return np.stack([x, y, z], 1).astype(dt)


def rough_transmittance(sl, cos, dt):
    """a rough-transmittance slice (n samples over cos^(1/4), then the diffuse transmittance) at cos theta: cubic Hermite interpolation
    with central-difference slopes (one-sided at the ends), clamped to [0, 1]"""
    v = np.asarray(sl, dt)[:-1]
    n = len(v)
    cos = np.asarray(cos, dt)
    x = np.power(np.abs(cos), dt(0.25))
    t = x * dt(n - 1)
    k = np.clip(t.astype(np.int64), 0, n - 2)
    f0, f1 = v[k], v[k + 1]
    d0 = np.where(k > 0, dt(0.5) * (v[k + 1] - v[np.maximum(k - 1, 0)]), v[k + 1] - v[k])
    d1 = np.where(k + 2 < n, dt(0.5) * (v[np.minimum(k + 2, n - 1)] - v[k]), v[k + 1] - v[k])
    t = t - k.astype(dt)
    t2 = t * t
    t3 = t2 * t
    r = (dt(2) * t3 - dt(3) * t2 + dt(1)) * f0 + (dt(-2) * t3 + dt(3) * t2) * f1 + (t3 - dt(2) * t2 + t) * d0 + (t3 - t2) * d1
    r = np.where((x >= 0) & (x <= 1), r, dt(0))
    return np.where(cos >= 0, np.minimum(dt(1), np.maximum(dt(0), r)), dt(0)).astype(dt)


def realloc(p, w, dt):
    return (p * w) / (p * w + (dt(1) - p) * (dt(1) - w))


# Total internal reflection on the way out is decided by the sign of 1 - s, s = eta^2 sin^2 theta', and the direction that leaves has
# cos theta = sqrt(1 - s): its relative error is that of s — a few 2^-24 in float32 — divided by 2 (1 - s).  So the distance to this branch
# point counts a tenth: at the exclusion threshold of 1e-4 (test 4) 1 - s is 1e-3, the outgoing cosine 0.03, and the rounding of s is
# amplified 500 times, to the 1e-4 that the sharpest lobes make of a float32 direction anyway.  Nearer the critical angle the outgoing
# direction of ANY float32 implementation is decided by the last bits of s.
TIR_SCALE = 0.1


class Sample:
    """what sample() returns, per item: direction, density, weight (all zero where the sample failed) and the delta flag; `margin`: the
    distance of the item to the nearest branch point on the way (lobe choices in units of the random number, side checks in units of the
    cosine, total internal reflection in units of 10 sin^2: TIR_SCALE)"""

    def __init__(self, wo, pdf, weight, delta, margin):
        self.wo, self.pdf, self.weight, self.delta, self.margin = wo, pdf, weight, delta, margin

    def cleaned(self, dt):
        with np.errstate(all="ignore"):  # (a sample that is not finite has failed: roughcoating's own lobe from below a one-sided surface)
            ok = self.weight.any(1) & (self.pdf != 0) & np.isfinite(self.pdf) & np.isfinite(self.weight).all(1) & np.isfinite(self.wo).all(1)
        z = ~ok
        self.wo = np.where(z[:, None], dt(0), self.wo)
        self.pdf = np.where(z, dt(0), self.pdf)
        self.weight = np.where(z[:, None], dt(0), self.weight)
        self.delta = self.delta & ok
        return self


class Leaf:
    """one of the BSDFs a coat may wrap, one-sided; eval() is f |cos theta_o| in the solid-angle measure (nothing for a delta component)"""

    def __init__(self, mat, dt=np.float64):
        self.dt, self.type = dt, mat["type"]
        three = lambda v, d: np.asarray([v] * 3 if np.isscalar(v) else v, f32).astype(dt) if v is not None else np.full(3, d, dt)  # noqa: E731
        self.refl = three(mat.get("reflectance"), 0.5)
        self.spec = three(mat.get("specular"), 1.0)
        self.lum = np.asarray(LUM, f32).astype(dt)
        if self.type in ("conductor", "roughconductor"):
            self.eta, self.k = three(mat["eta"], 0), three(mat["k"], 1)
        if self.type in ("plastic", "roughplastic"):
            self.eta = dt(f32(mat["eta"]))
            d_avg, s_avg = (self.refl * self.lum).sum(), (self.spec * self.lum).sum()
            self.w = s_avg / (d_avg + s_avg)
        if self.type == "plastic":
            self.fdr = dt(f32(diffuse_fresnel_reflectance(1.0 / float(f32(mat["eta"])))))
        if self.type in ("roughconductor", "roughplastic"):
            self.distr = Distribution(mat.get("distribution", "ggx"), f32(mat["alpha"]), f32(mat["alpha"]), dt)
        if self.type == "roughplastic":
            self.slice = np.asarray(mat["slice"], f32)
            self.fdr = dt(1) - dt(self.slice[-1])
        self.has_delta = self.type in ("conductor", "plastic")

    def _diff(self):
        return self.refl / (self.dt(1) - self.fdr)

    def _ps(self, wi):
        dt = self.dt
        if self.type == "plastic":
            p = fresnel_dielectric(wi[:, 2], self.eta, dt)[0]
        else:
            p = dt(1) - rough_transmittance(self.slice, wi[:, 2], dt)
        return realloc(p, self.w, dt)

    def eval(self, wi, wo):
        dt = self.dt
        wi, wo = _v(wi, dt), _v(wo, dt)
        ok = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        inv_pi = dt(1) / dt(np.pi)
        with np.errstate(all="ignore"):
            if self.type == "diffuse":
                r = self.refl[None] * (inv_pi * wo[:, 2])[:, None]
            elif self.type == "conductor":
                r = np.zeros_like(wo)
            elif self.type == "roughconductor":
                h = normalize(wo + wi)
                model = self.distr.D(h) * (self.distr.G1(wi, h) * self.distr.G1(wo, h)) / (dt(4) * wi[:, 2])
                r = fresnel_conductor(dot(wi, h), self.eta, self.k, dt) * self.refl[None] * model[:, None]
            elif self.type == "plastic":
                fi, fo = fresnel_dielectric(wi[:, 2], self.eta, dt)[0], fresnel_dielectric(wo[:, 2], self.eta, dt)[0]
                r = self._diff()[None] * ((inv_pi * wo[:, 2]) / (self.eta * self.eta) * (dt(1) - fi) * (dt(1) - fo))[:, None]
            else:
                h = normalize(wo + wi)
                f = fresnel_dielectric(dot(wi, h), self.eta, dt)[0]
                value = f * self.distr.D(h) * (self.distr.G1(wi, h) * self.distr.G1(wo, h)) / (dt(4) * wi[:, 2])
                t12, t21 = rough_transmittance(self.slice, wi[:, 2], dt), rough_transmittance(self.slice, wo[:, 2], dt)
                r = self.spec[None] * value[:, None] + self._diff()[None] * (inv_pi * wo[:, 2] * t12 * t21 / (self.eta * self.eta))[:, None]
        return np.where(ok[:, None], r, dt(0)).astype(dt)

    def pdf(self, wi, wo):
        dt = self.dt
        wi, wo = _v(wi, dt), _v(wo, dt)
        ok = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        inv_pi = dt(1) / dt(np.pi)
        with np.errstate(all="ignore"):
            if self.type == "diffuse":
                r = inv_pi * wo[:, 2]
            elif self.type == "conductor":
                r = np.zeros(len(wo), dt)
            elif self.type == "roughconductor":
                h = normalize(wo + wi)
                r = self.distr.D(h) * self.distr.G1(wi, h) / (dt(4) * wi[:, 2])
            elif self.type == "plastic":
                r = (inv_pi * wo[:, 2]) * (dt(1) - self._ps(wi))
            else:
                h = normalize(wo + wi)
                ps = self._ps(wi)
                r = self.distr.pdf_visible(wi, h) / (dt(4) * dot(wo, h)) * ps + (dt(1) - ps) * (inv_pi * wo[:, 2])
        return np.where(ok, r, dt(0)).astype(dt)

    def sample(self, wi, u):
        dt = self.dt
        wi, u = _v(wi, dt), np.asarray(u, dt).reshape(-1, 2)
        n = len(u)
        up = wi[:, 2] > 0
        big = np.full(n, np.inf)
        delta = np.zeros(n, bool)
        inv_pi = dt(1) / dt(np.pi)
        safe = np.where(up[:, None], wi, np.asarray([0, 0, 1], dt)[None])
        with np.errstate(all="ignore"):
            if self.type == "diffuse":
                wo = cosine_hemisphere(u, dt)
                pdf = inv_pi * wo[:, 2]
                w = np.broadcast_to(self.refl[None], (n, 3))
                margin = big
            elif self.type == "conductor":
                wo = safe * np.asarray([-1, -1, 1], dt)[None]
                pdf = np.ones(n, dt)
                w = self.refl[None] * fresnel_conductor(safe[:, 2], self.eta, self.k, dt)
                delta = np.ones(n, bool)
                margin = big
            elif self.type == "roughconductor":
                m = self.distr.sample_visible(safe, u)
                pm = self.distr.pdf_visible(safe, m)
                wo = m * (dt(2) * dot(safe, m))[:, None] - safe
                w = fresnel_conductor(dot(safe, m), self.eta, self.k, dt) * self.refl[None] * self.distr.G1(wo, m)[:, None]
                pdf = pm / (dt(4) * dot(wo, m))
                bad = (pm == 0) | (wo[:, 2] <= 0)
                w, pdf = np.where(bad[:, None], dt(0), w), np.where(bad, dt(0), pdf)
                margin = np.abs(wo[:, 2]).astype(np.float64)
            elif self.type == "plastic":
                fi = fresnel_dielectric(safe[:, 2], self.eta, dt)[0]
                ps = self._ps(safe)
                spec = u[:, 0] < ps
                ud = np.stack([(u[:, 0] - ps) / (dt(1) - ps), u[:, 1]], 1)
                wd = cosine_hemisphere(np.where(spec[:, None], dt(0.5), ud), dt)
                fo = fresnel_dielectric(wd[:, 2], self.eta, dt)[0]
                wo = np.where(spec[:, None], safe * np.asarray([-1, -1, 1], dt)[None], wd)
                pdf = np.where(spec, ps, (dt(1) - ps) * (inv_pi * wd[:, 2]))
                w = np.where(spec[:, None], self.spec[None] * (fi / ps)[:, None],
                             self._diff()[None] * ((dt(1) - fi) * (dt(1) - fo) / (self.eta * self.eta) / (dt(1) - ps))[:, None])
                delta = spec
                margin = np.abs(u[:, 0] - ps).astype(np.float64)
            else:
                ps = self._ps(safe)
                spec = u[:, 1] < ps
                us = np.stack([u[:, 0], u[:, 1] / ps], 1)
                ud = np.stack([u[:, 0], (u[:, 1] - ps) / (dt(1) - ps)], 1)
                m = self.distr.sample_visible(safe, np.where(spec[:, None], us, dt(0.5)))
                ws = m * (dt(2) * dot(safe, m))[:, None] - safe
                wo = np.where(spec[:, None], ws, cosine_hemisphere(np.where(spec[:, None], dt(0.5), ud), dt))
                bad = spec & (ws[:, 2] <= 0)
                wo = np.where(bad[:, None], np.asarray([0, 0, 1], dt)[None], wo)
                pdf = self.pdf(safe, wo)
                w = self.eval(safe, wo) / pdf[:, None]
                bad = bad | (pdf == 0)
                w, pdf = np.where(bad[:, None], dt(0), w), np.where(bad, dt(0), pdf)
                margin = np.minimum(np.abs(u[:, 1] - ps), np.where(spec, np.abs(ws[:, 2]), np.inf)).astype(np.float64)
        w = np.where(up[:, None], w, dt(0))
        pdf = np.where(up, pdf, dt(0))
        return Sample(wo.astype(dt), pdf.astype(dt), w.astype(dt), delta & up, np.where(up, margin, np.inf)).cleaned(dt)


class Coat:
    """`coating` / `roughcoating` around a Leaf, optionally inside a two-sided adapter"""

    def __init__(self, coat, leaf, twosided=False, dt=np.float64):
        self.dt, self.leaf, self.twosided = dt, Leaf(leaf, dt) if isinstance(leaf, dict) else leaf, twosided
        c = Coating.from_dict({k: v for k, v in coat.items() if k != "slice"})  # (the host's view of the dict: defaults and float32 rounding)
        self.rough = c.kind == 2
        self.eta = dt(f32(c.eta))
        self.inv_eta = dt(1) / self.eta
        self.thickness = dt(f32(c.thickness))
        self.sigma_a = np.asarray(list(c.sigma_a), f32).astype(dt)
        self.spec = np.asarray(list(c.specular), f32).astype(dt)
        # the sampling weight of the layer's own component is derived once, in float32, by every host alike
        s32 = np.asarray(list(c.sigma_a), f32)
        self.ssw = dt(f32(1) / (np.exp(s32.astype(np.float64) * float(f32(-2) * f32(c.thickness))).astype(f32).sum(dtype=f32) * f32(1.0 / 3) + f32(1)))
        if self.rough:
            kind = {0: "beckmann", 1: "ggx", 2: "phong"}[c.distribution]
            self.sample_all = bool(c.sample_all) or kind == "phong"
            self.distr = Distribution(kind, f32(c.alpha), f32(c.alpha), dt)
            self.slice = np.asarray(coat["slice"], f32)

    # -- the layer
    def refract_in(self, w, out=False):
        """through the smooth boundary (out = True: from the inside), keeping the side of the direction: (direction, reflectance)"""
        dt = self.dt
        eta, inv = (self.inv_eta, self.eta) if out else (self.eta, self.inv_eta)
        r, ct = fresnel_dielectric(np.abs(w[:, 2]), eta, dt)
        sgn = np.where(np.signbit(w[:, 2]), dt(-1), dt(1))
        return np.stack([inv * w[:, 0], inv * w[:, 1], -sgn * ct], 1).astype(dt), r

    def refract_to(self, w, inv_eta):
        """Snell's law alone, for the rough boundary: the zero vector on total internal reflection; and the distance to that case"""
        dt = self.dt
        s2 = inv_eta * inv_eta * (dt(1) - w[:, 2] * w[:, 2])
        tir = s2 >= 1
        ct = np.sqrt(np.maximum(dt(1) - s2, dt(0)))
        r = np.stack([inv_eta * w[:, 0], inv_eta * w[:, 1], np.where(w[:, 2] > 0, ct, -ct)], 1)
        return np.where(tir[:, None], dt(0), r).astype(dt), np.abs(s2 - dt(1)).astype(np.float64)

    def absorption(self, ci, co):
        dt = self.dt
        s = self.sigma_a * self.thickness
        if not s.any():
            return np.ones((len(ci), 3), dt)
        with np.errstate(all="ignore"):
            t = dt(1) / np.abs(ci) + dt(1) / np.abs(co)
            return np.exp(-s[None] * t[:, None]).astype(dt)

    def T(self, c):
        return rough_transmittance(self.slice, np.abs(c), self.dt)

    def prob_specular(self, wi):
        dt = self.dt
        p = self.refract_in(wi)[1] if not self.rough else dt(1) - self.T(wi[:, 2])
        return realloc(p, self.ssw, dt)

    def _flip(self, wi, *vs):
        dt = self.dt
        s = np.where(self.twosided & ~(wi[:, 2:3] > 0), dt(-1), dt(1))
        k = np.concatenate([np.ones_like(s), np.ones_like(s), s], 1)
        return [v * k for v in (wi,) + vs]

    # -- the plug-ins
    def eval(self, wi, wo, parts=False):
        dt = self.dt
        wo = _v(wo, dt)
        wi = np.broadcast_to(_v(wi, dt), wo.shape)
        return self._eval(*self._flip(wi, wo), parts=parts)

    def pdf(self, wi, wo):
        dt = self.dt
        wo = _v(wo, dt)
        wi = np.broadcast_to(_v(wi, dt), wo.shape)
        return self._pdf(*self._flip(wi, wo))

    def _eval(self, wi, wo, parts=False):
        dt = self.dt
        with np.errstate(all="ignore"):
            if not self.rough:
                wip, r12 = self.refract_in(wi)
                wop, r21 = self.refract_in(wo)
                dead = (r12 == 1) | (r21 == 1)
                a, b = dt(1) - r12, dt(1) - r21
                own = np.zeros_like(wo)
            else:
                same = wo[:, 2] * wi[:, 2] > 0
                h = normalize(wo + wi) * np.where(np.signbit(wo[:, 2]), dt(-1), dt(1))[:, None]
                f = fresnel_dielectric(np.abs(dot(wi, h)), self.eta, dt)[0]
                value = f * self.distr.D(h) * (self.distr.G1(wi, h) * self.distr.G1(wo, h)) / (dt(4) * np.abs(wi[:, 2]))
                own = np.where(same[:, None], self.spec[None] * value[:, None], dt(0))
                wip, _ = self.refract_to(wi, self.inv_eta)
                wop, _ = self.refract_to(wo, self.inv_eta)
                dead = ~wip.any(1) | ~wop.any(1)
                a, b = self.T(wi[:, 2]), self.T(wo[:, 2])
            nested = self.leaf.eval(wip, wop) * a[:, None] * b[:, None] * self.absorption(wip[:, 2], wop[:, 2])
            nested = nested * (self.inv_eta * self.inv_eta * wo[:, 2] / wop[:, 2])[:, None]
            nested = np.where(dead[:, None], dt(0), nested)
        return (own.astype(dt), nested.astype(dt)) if parts else (own + nested).astype(dt)

    def _pdf(self, wi, wo):
        dt = self.dt
        ps = self.prob_specular(wi)
        with np.errstate(all="ignore"):
            if not self.rough:
                wip, r12 = self.refract_in(wi)
                wop, r21 = self.refract_in(wo)
                dead = (r12 == 1) | (r21 == 1)
                own = np.zeros(len(wo), dt)
            else:
                same = wo[:, 2] * wi[:, 2] > 0
                h = normalize(wo + wi) * np.where(np.signbit(wo[:, 2]), dt(-1), dt(1))[:, None]
                own = np.where(same, self.distr.pdf(wi, h, self.sample_all) / (dt(4) * np.abs(dot(wo, h))) * ps, dt(0))
                wip, _ = self.refract_to(wi, self.inv_eta)
                wop, _ = self.refract_to(wo, self.inv_eta)
                dead = ~wip.any(1) | ~wop.any(1)
            nested = self.leaf.pdf(wip, wop) * (self.inv_eta * self.inv_eta * wo[:, 2] / wop[:, 2]) * (dt(1) - ps)
            nested = np.where(dead, dt(0), nested)
        return (own + nested).astype(dt)

    def sample(self, wi, u):
        dt = self.dt
        u = np.asarray(u, dt).reshape(-1, 2)
        n = len(u)
        wi0 = np.broadcast_to(_v(wi, dt), (n, 3))
        wi, = self._flip(wi0)
        flipped = wi[:, 2] != wi0[:, 2]
        ps = self.prob_specular(wi)
        sel = u[:, 1] if self.rough else u[:, 0]
        own = sel < ps
        margin = np.abs(sel - ps).astype(np.float64)
        with np.errstate(all="ignore"):
            rest = (sel - ps) / (dt(1) - ps)
            if not self.rough:
                wip, r12 = self.refract_in(wi)
                s = self.leaf.sample(wip, np.stack([np.where(own, dt(0.5), rest), u[:, 1]], 1))
                wo, r21 = self.refract_in(s.wo, out=True)
                margin = np.where(own, margin, np.minimum(margin, np.minimum(s.margin, TIR_SCALE * np.abs(self.eta * self.eta * (1 - s.wo[:, 2] ** 2) - 1))))
                w = s.weight * self.absorption(wip[:, 2], s.wo[:, 2]) / (dt(1) - ps)[:, None] * ((dt(1) - r12) * (dt(1) - r21))[:, None]
                pdf = s.pdf * (dt(1) - ps) * np.where(s.delta, dt(1), self.inv_eta * self.inv_eta * wo[:, 2] / s.wo[:, 2])
                dead = (r12 == 1) | (r21 == 1) | ~s.weight.any(1)
                w, pdf = np.where(dead[:, None], dt(0), w), np.where(dead, dt(0), pdf)
                wo = np.where(own[:, None], wi * np.asarray([-1, -1, 1], dt)[None], wo)
                pdf = np.where(own, ps, pdf)
                w = np.where(own[:, None], self.spec[None] * (r12 / ps)[:, None], w)
                delta = own | s.delta
            else:
                m, _ = self.distr.sample(wi, np.stack([u[:, 0], np.where(own, sel / ps, dt(0.5))], 1), self.sample_all)
                wr = m * (dt(2) * dot(wi, m))[:, None] - wi
                wip, _ = self.refract_to(wi, self.inv_eta)
                s = self.leaf.sample(wip, np.stack([u[:, 0], np.where(own, dt(0.5), rest)], 1))
                wout, tir = self.refract_to(s.wo, self.eta)
                dead = np.where(own, wr[:, 2] * wi[:, 2] <= 0, ~wip.any(1) | ~s.weight.any(1) | ~wout.any(1))
                margin = np.minimum(margin, np.where(own, np.abs(wr[:, 2]), np.minimum(s.margin, TIR_SCALE * tir)))
                wo = np.where(dead[:, None], np.asarray([0, 0, 1], dt)[None] * np.where(wi[:, 2:3] > 0, dt(1), dt(-1)), np.where(own[:, None], wr, wout))
                pdf = self._pdf(wi, wo)
                w = self._eval(wi, wo) / pdf[:, None]
                dead = dead | (pdf == 0)
                w, pdf = np.where(dead[:, None], dt(0), w), np.where(dead, dt(0), pdf)
                delta = np.zeros(n, bool)
        out = Sample(wo.astype(dt), pdf.astype(dt), w.astype(dt), delta, margin).cleaned(dt)
        out.wo = np.where((flipped & out.weight.any(1))[:, None], out.wo * np.asarray([1, 1, -1], dt)[None], out.wo)
        return out


# ------------------------------------------------------------------------------------------------ 1. the closed form
def _hemisphere(n_theta, n_phi=8):
    th = (np.arange(n_theta) + 0.5) / n_theta * (np.pi / 2)
    ph = (np.arange(n_phi) + 0.5) / n_phi * 2 * np.pi
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(TH) * np.cos(PH), np.sin(TH) * np.sin(PH), np.cos(TH)], -1).reshape(-1, 3)
    return d, (np.sin(TH) * (np.pi / 2 / n_theta) * (2 * np.pi / n_phi)).reshape(-1)


@pytest.mark.parametrize("eta", [1.5, 1.9])
@pytest.mark.parametrize("sigma_a", [(0, 0, 0), (0.4, 0.1, 0.02)], ids=["clear", "tinted"])
@pytest.mark.parametrize("wname", ["normal", "oblique", "grazing"])
def test_coated_diffuse_pdf_integrates_to_the_escaping_fraction(eta, sigma_a, wname):
    """A cosine-distributed direction under the layer leaves it unless it is totally reflected: with probability sin^2 theta_c = 1 / eta^2.
    So the density of coating over diffuse integrates to (1 - probSpecular) / eta^2 over the upper hemisphere, whatever sigmaA is — which
    pins the Jacobian eta^-2 cos theta_o / cos theta_o' and the cut at the critical angle.  The quadrature's error is what halving its
    step shows."""
    c = Coat(dict(SMOOTH_COAT, eta=eta, sigma_a=sigma_a), DIFFUSE)
    wi = unit(WIS[wname]).astype(np.float64)[None]
    want = float((1 - c.prob_specular(wi)[0]) / float(f32(eta)) ** 2)
    totals = []
    for n in (2000, 4000):
        d, dw = _hemisphere(n)
        totals.append(float((c.pdf(wi, d) * dw).sum()))
    err = abs(totals[1] - totals[0])
    print("integral", totals, "closed form", want, "quadrature error", err)
    assert err < 1e-5 * want
    assert abs(totals[1] - want) <= 2 * err + 1e-12


# ------------------------------------------------------------------------------------------------ 2. sample() against eval() and pdf()
def _lattice_u(n):
    i, j = np.divmod(np.arange(n * n), n)
    return np.stack([(i + 0.5) / n, (j + 0.37) / n], 1)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
@pytest.mark.parametrize("wname", list(WIS))
def test_sample_is_consistent_with_eval_and_pdf(case, wname):
    cname, nname, twosided = case
    c = Coat(coat_of(cname), NESTED[nname], twosided)
    wi = unit(WIS[wname]).astype(np.float64)
    s = c.sample(wi, _lattice_u(96))
    ok = s.weight.any(1)
    if wi[2] < 0 and not twosided and c.rough:
        # From behind a one-sided roughcoating only its own lobe answers.  (Its sample() draws a visible normal for a direction below
        # the surface, which means nothing: what comes back is finite or a failed sample, and is not looked at further.)
        _, wo, _ = lattice(False)
        own, nested = c.eval(wi, wo, parts=True)
        assert not nested.any() and own[wo[:, 2] < 0].any() and np.isfinite(own).all() and np.isfinite(c.pdf(wi, wo)).all()
        assert np.isfinite(s.weight).all() and np.isfinite(s.pdf).all()
        return
    assert ok.any()
    sm = ok & ~s.delta
    if sm.any():
        f, p = c.eval(wi, s.wo[sm]), c.pdf(wi, s.wo[sm])
        assert np.all(p > 0)
        assert np.allclose(s.pdf[sm], p, rtol=1e-9, atol=1e-300)
        assert np.allclose(s.weight[sm] * s.pdf[sm][:, None], f, rtol=1e-9, atol=1e-300)
    wi1 = np.array([wi * ([1, 1, -1] if twosided and wi[2] < 0 else [1, 1, 1])])  # in the two-sided adapter's frame
    own = (_lattice_u(96)[:, 0] < c.prob_specular(wi1)[0]) if not c.rough else np.zeros(len(ok), bool)
    assert np.all(s.delta[own]) and np.all(ok[own])
    if own.any():  # the layer's delta reflection: weight * pdf = specularReflectance * Fresnel, pdf = probSpecular
        r = fresnel_dielectric(abs(wi[2]), c.eta, np.float64)[0]
        assert np.allclose(s.weight[own] * s.pdf[own][:, None], c.spec[None] * r)
        assert np.allclose(s.pdf[own], c.prob_specular(wi1)[0]) and np.allclose(s.wo[own], wi * [-1, -1, 1])
    nested_delta = ok & s.delta & ~own
    assert nested_delta.any() == (c.leaf.has_delta and (wi[2] > 0 or twosided))


CHI2_SIGNIFICANCE = 0.01  # test_chisquare.cpp's significance level (ChiSquare::runTest's default)


@pytest.mark.parametrize("case", [c for c in CASES if not c[2]], ids=[case_id(c) for c in CASES if not c[2]])
def test_sampled_directions_follow_the_pdf(case):
    """test_chisquare.cpp's check: a histogram of sampled directions against the integral of pdf() per bin, Pearson's chi-square at the
    reference's significance level, bins with an expected count below 5 pooled as the reference pools them"""
    from scipy import stats
    cname, nname, _ = case
    c = Coat(coat_of(cname), NESTED[nname])
    wi = unit(WIS["oblique"]).astype(np.float64)
    rng = np.random.RandomState(3)
    n = 200000
    s = c.sample(wi, rng.rand(n, 2))
    sm = s.weight.any(1) & ~s.delta
    if not sm.any():
        assert nname == "copper"  # all components are delta
        return
    nb_t, nb_p, sub = 10, 20, 24
    th = (np.arange(nb_t * sub) + 0.5) / (nb_t * sub) * (np.pi / 2)
    ph = (np.arange(nb_p * sub) + 0.5) / (nb_p * sub) * 2 * np.pi
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(TH) * np.cos(PH), np.sin(TH) * np.sin(PH), np.cos(TH)], -1).reshape(-1, 3)
    dw = np.sin(TH) * (np.pi / 2 / (nb_t * sub)) * (2 * np.pi / (nb_p * sub))
    expect = (c.pdf(wi, d).reshape(TH.shape) * dw).reshape(nb_t, sub, nb_p, sub).sum((1, 3)) * n
    w = s.wo[sm]
    it = np.clip((np.arccos(np.clip(w[:, 2], -1, 1)) / (np.pi / 2) * nb_t).astype(int), 0, nb_t - 1)
    ip = np.clip(((np.arctan2(w[:, 1], w[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nb_p).astype(int), 0, nb_p - 1)
    obs = np.zeros((nb_t, nb_p))
    np.add.at(obs, (it, ip), 1)
    obs, expect = obs.ravel(), expect.ravel()
    # the draws that gave no smooth sample (the delta lobes, failed samples) form one more cell
    obs, expect = np.append(obs, n - sm.sum()), np.append(expect, n - expect.sum())
    order = np.argsort(expect)
    obs, expect = obs[order], expect[order]
    pooled = np.cumsum(expect) < 5
    o = np.append(obs[~pooled], obs[pooled].sum()) if pooled.any() else obs
    e = np.append(expect[~pooled], expect[pooled].sum()) if pooled.any() else expect
    keep = e > 0
    chi2 = float((((o - e) ** 2)[keep] / e[keep]).sum())
    dof = int(keep.sum()) - 1
    p = float(stats.chi2.sf(chi2, dof))
    print("chi2", chi2, "dof", dof, "p", p)
    assert p >= CHI2_SIGNIFICANCE


# ------------------------------------------------------------------------------------------------ 3. the limits
def _pairs(n=500, seed=5):
    rng = np.random.RandomState(seed)
    a = rng.randn(n, 3); a[:, 2] = np.abs(a[:, 2]) + 0.1; a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.randn(n, 3); b[:, 2] = np.abs(b[:, 2]) + 0.1; b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b


@pytest.mark.parametrize("nname", list(NESTED))
def test_a_clear_layer_of_index_one_is_no_layer(nname):
    """eval tends to the nested eval as eta -> 1: the difference is of first order in eta - 1 (the refracted directions move by
    (eta - 1) tan theta, the transmittances by its square; a glossy lobe of roughness alpha answers with a relative change of about
    (eta - 1) tan theta / alpha^2, a few hundred times eta - 1 here), so it is below 1e-3 at 1 + 1e-6 and ten times smaller than at 1 + 1e-5"""
    a, b = _pairs()
    want = Leaf(NESTED[nname]).eval(a, b)
    err = []
    for d in (1e-5, 1e-6):
        c = Coat(dict(kind="coating", eta=np.float64(1 + d), sigma_a=0.0), NESTED[nname])
        c.eta, c.inv_eta = np.float64(1 + d), 1 / np.float64(1 + d)  # (not rounded to float32: 1 + 1e-6 is 8 float32 steps from 1)
        err.append(float(np.abs(c.eval(a, b) - want).max() / max(np.abs(want).max(), 1e-300)))
    print("largest deviation relative to the largest value, eta - 1 = 1e-5, 1e-6:", err)
    assert err[1] < 1e-3
    assert err[1] <= 0.11 * err[0] + 1e-15


@pytest.mark.parametrize("cname", ["coating", "roughcoating-ggx", "roughcoating-beckmann"])
def test_without_specular_reflectance_the_layer_reflects_nothing_itself(cname):
    a, b = _pairs()
    c = Coat(dict(coat_of(cname), specular=0.0), DIFFUSE)
    own, nested = c.eval(a, b, parts=True)
    assert not own.any() and nested.any()
    s = c.sample(a, _lattice_u(23)[:len(a)])
    mine = s.delta if not c.rough else np.zeros(len(a), bool)
    assert not s.weight[mine].any()
    full = Coat(coat_of(cname), DIFFUSE)
    assert np.array_equal(full.eval(a, b, parts=True)[1], nested)


@pytest.mark.parametrize("cname", ["coating", "roughcoating-ggx"])
def test_absorption_is_exactly_the_stated_exponential(cname):
    a, b = _pairs()
    coat = coat_of(cname)
    tinted, clear = Coat(coat, GOLD), Coat(dict(coat, sigma_a=0.0), GOLD)
    ci = np.sqrt(1 - (1 - a[:, 2] ** 2) / float(f32(coat["eta"])) ** 2)
    co = np.sqrt(1 - (1 - b[:, 2] ** 2) / float(f32(coat["eta"])) ** 2)
    s = np.asarray(coat["sigma_a"], f32).astype(np.float64) * float(f32(coat["thickness"]))
    want = clear.eval(a, b, parts=True)[1] * np.exp(-s[None] * (1 / ci + 1 / co)[:, None])
    assert np.allclose(tinted.eval(a, b, parts=True)[1], want, rtol=1e-12, atol=0)
    assert np.array_equal(tinted.eval(a, b, parts=True)[0], clear.eval(a, b, parts=True)[0])


# ------------------------------------------------------------------------------------------------ 4. float32 against float64
N = 4096
MARGIN = 1e-4         # an item closer than this to a branch point (Sample.margin) is left out of the comparison ...
MAX_EXCLUDED = 0.005  # ... and no case may lose more than this share of its items
VALUE_FLOOR = 1e-2    # deviations of eval / pdf / weight are relative to max(|reference|, VALUE_FLOOR)


def lattice(twosided):
    """4096 items: u the first points of the rank-1 lattice frac(0.5 + k (0.7548776662, 0.5698402910)) (no two items share a
    coordinate, so a branch point costs the rule a strip and not a column), squeezed into [1e-3, 1 - 1e-3]; wo on a lattice of the sphere
    (|cos| from 0.03 up); and the four wi of test_bsdfs.py — normal, oblique, grazing (cos = 0.084), from below — taking turns.  A case
    without the two-sided adapter sees the last one from above: from below its BSDF has nothing to compare."""
    k = np.arange(N)
    i, j = np.divmod(k, 64)
    u = (1e-3 + np.modf(0.5 + k[:, None] * np.array([0.7548776662, 0.5698402910])[None])[0] * (1 - 2e-3)).astype(f32)
    wi = np.stack([unit(w) for w in WIS.values()])[(i + j) % 4]
    if not twosided:
        wi[:, 2] = np.abs(wi[:, 2])
    cz = (((j + 0.5) / 64) * 2 - 1) * 0.97
    cz = np.where(np.abs(cz) < 0.03, 0.03, cz)
    ph = 2 * np.pi * (i + 0.37) / 64
    wo = np.stack([np.sqrt(1 - cz * cz) * np.cos(ph), np.sqrt(1 - cz * cz) * np.sin(ph), cz], 1)
    return wi.astype(f32), (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(f32), u


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), VALUE_FLOOR)


def reference(case):
    """the float64 restatement over the lattice: eval, pdf, the sample, and the items the exclusion rule leaves in"""
    cname, nname, twosided = case
    wi, wo, u = lattice(twosided)
    c = Coat(coat_of(cname), NESTED[nname], twosided)
    s = c.sample(wi, u)
    return dict(eval=c.eval(wi, wo), pdf=c.pdf(wi, wo), sample=s, keep=s.margin >= MARGIN)


def deviations(got, ref):
    """largest deviation of eval, pdf, weight and sampled direction from the float64 reference; the sample's over the kept items on
    which both sides produced one"""
    keep = ref["keep"]
    s, g = ref["sample"], got["sample"]
    both = keep & s.weight.any(1) & np.asarray(g.weight).any(1)
    return dict(eval=float(rel(got["eval"], ref["eval"]).max()), pdf=float(rel(got["pdf"], ref["pdf"]).max()),
                weight=float(rel(np.asarray(g.weight)[both], s.weight[both]).max()) if both.any() else 0.0,
                sampled_pdf=float(rel(np.asarray(g.pdf)[both], s.pdf[both]).max()) if both.any() else 0.0,
                direction=float(angle(np.asarray(g.wo)[both], s.wo[both]).max()) if both.any() else 0.0)


_f32_cache = {}


def float32_figures(case):
    """(deviations of the float32 restatement from the float64 one, share of items excluded, share of kept items on which the two
    precisions take different branches)"""
    if case not in _f32_cache:
        cname, nname, twosided = case
        wi, wo, u = lattice(twosided)
        c = Coat(coat_of(cname), NESTED[nname], twosided, f32)
        got = dict(eval=c.eval(wi, wo), pdf=c.pdf(wi, wo), sample=c.sample(wi, u))
        assert got["eval"].dtype == f32 and got["sample"].wo.dtype == f32
        ref = reference(case)
        s, g = ref["sample"], got["sample"]
        keep = ref["keep"]
        differ = keep & ((s.weight.any(1) != g.weight.any(1)) | (s.delta != g.delta))
        _f32_cache[case] = (deviations(got, ref), float(1 - keep.mean()), float(differ.sum() / max(1, keep.sum())))
    return _f32_cache[case]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_float32_restatement_against_float64(case):
    """The figures the GPU test's bounds come from.  Outside the exclusion rule (an item within MARGIN of a lobe choice, of total internal
    reflection or of a side check) the two precisions must take the same branches, and the rule may cost a case at most 0.5 % of its items."""
    dev, excluded, differ = float32_figures(case)
    print(case_id(case), "float32 vs float64:", dev, "excluded", excluded, "different branches among the kept", differ)
    assert excluded <= MAX_EXCLUDED
    assert differ == 0
    assert all(np.isfinite(v) for v in dev.values())
    wi, _, _ = lattice(case[2])
    assert (np.abs(wi[:, 2]) < 0.1).any() and (wi[:, 2] < 0).any() == case[2]  # grazing wi, and wi from below under twosided


# ------------------------------------------------------------------------------------------------ 5. the hosts
def test_oracle_binding_refuses_coatings(oracle_lib):
    from conftest import CBOX_PROPS, make_oracle
    desc = ppg_host.cbox_scene(16, 12)
    desc.materials = list(desc.materials) + [dict(DIFFUSE, coating=dict(SMOOTH_COAT))]
    o = make_oracle(oracle_lib, **dict(CBOX_PROPS, budget=4))
    with pytest.raises(NotImplementedError):
        o.set_scene(desc)


from test_microfacet_general import REF_DATA, SPHERE, _cpp, _material_records, _save, _scene  # noqa: E402

needs_tables = pytest.mark.skipif(not os.path.exists(os.path.join(REF_DATA, "microfacet", "ggx.dat")), reason="needs Mitsuba's data/microfacet tables")
NONE = '<string name="material" value="none"/>'
COAT_XML = {
    "twosided-coating-roughconductor": (
        '<bsdf type="twosided"> <bsdf type="coating"> <float name="intIOR" value="1.7"/> <float name="thickness" value="2"/> <rgb name="sigmaA" value="0.1, 0.2, 0.3"/>'
        ' <bsdf type="roughconductor"> %s <string name="distribution" value="ggx"/> <float name="alpha" value="0.25"/> </bsdf> </bsdf> </bsdf>' % NONE,
        dict(type=4, twosided=True, alpha=0.25),
        dict(kind="coating", eta=float(f32(1.7 / 1.000277)), thickness=2.0, sigma_a=tuple(float(f32(v)) for v in (0.1, 0.2, 0.3)), specular=(1.0, 1.0, 1.0))),
    "coating-defaults-plastic": (
        '<bsdf type="coating"> <bsdf type="plastic"/> </bsdf>', dict(type=5),
        dict(kind="coating", eta=float(f32(1.5046 / 1.000277)), thickness=1.0, sigma_a=(0.0, 0.0, 0.0), specular=(1.0, 1.0, 1.0))),
    "roughcoating-roughplastic": (
        '<bsdf type="roughcoating"> <string name="distribution" value="ggx"/> <float name="alpha" value="0.1"/> <float name="intIOR" value="1.5"/> <float name="extIOR" value="1"/>'
        ' <rgb name="specularReflectance" value="0.5, 0.75, 1"/> <boolean name="sampleVisible" value="false"/>'
        ' <bsdf type="roughplastic"> <string name="distribution" value="beckmann"/> <float name="alpha" value="0.2"/> <float name="intIOR" value="1.49"/> <float name="extIOR" value="1"/> </bsdf> </bsdf>',
        dict(type=9, rtrans=0),
        dict(kind="roughcoating", eta=1.5, thickness=1.0, sigma_a=(0.0, 0.0, 0.0), specular=(0.5, 0.75, 1.0), alpha=float(f32(0.1)), distribution="ggx",
             sample_visible=False, slice=1)),
}


def _coat_bytes(desc):
    return b"".join(bytes(Coating.from_dict(m)) for m in desc.materials)


def _load(tmp_path, body, **kw):
    desc, _, info = ppg_host.load_scene(_scene(tmp_path, body), **kw)
    return desc, info


@needs_tables
@pytest.mark.parametrize("name", list(COAT_XML))
def test_both_loaders_read_the_coats_and_agree(tmp_path, name):
    """the Python loader's dicts; the C++ loader (ppg_render --ppgs, as tests/test_cpp_host.py runs it) writes the same ppg_material and
    ppg_coating records, the coatings as the file's last block (bit 12); the flat file gives the dicts back"""
    bsdf, want_m, want_c = COAT_XML[name]
    desc, info = _load(tmp_path, SPHERE % bsdf, data_dir=REF_DATA)
    assert not info["warnings"]
    m = desc.materials[desc.spheres[0]["material"]]
    for k, v in want_m.items():
        assert m[k] == v, (k, m)
    assert m["coating"] == want_c, m["coating"]
    if name == "roughcoating-roughplastic":  # two slices: the nested BSDF's own and the coat's, the golden ones
        assert np.array_equal(desc.rtrans[0], rtrans_slice("beckmann", 0.2, 1.49)) and np.array_equal(desc.rtrans[1], rtrans_slice("ggx", 0.1, 1.5))
    r, flat = _cpp(tmp_path, SPHERE % bsdf, "--data-dir", REF_DATA)
    assert r.returncode == 0, r.stderr
    mine = open(_save(desc, tmp_path), "rb").read()
    assert int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 4096 and int(np.frombuffer(mine, np.uint32, 6, 4)[5]) & 4096
    assert _material_records(flat) == _material_records(mine)
    coats = _coat_bytes(desc)
    assert len(coats) == 64 * len(desc.materials) and flat.endswith(coats) and mine.endswith(coats)
    back = ppg_host.load_scene_file(_save(desc, tmp_path))
    assert _coat_bytes(back) == coats and back.materials[desc.spheres[0]["material"]]["coating"]["kind"] == want_c["kind"]
    # ... and the XML writer
    again, _, info2 = ppg_host.load_scene(ppg_host.save_scene_xml(desc, dict(budgetType="spp", budget=8.0), str(tmp_path / "w")), data_dir=REF_DATA)
    assert not info2["warnings"] and _coat_bytes(again).count(bytes(Coating.from_dict(m))) == 1


def test_bumpmap_around_a_coating(tmp_path):
    from ppg_host import imageio
    imageio.write_pfm(str(tmp_path / "b.pfm"), np.linspace(0, 1, 48, dtype=f32).reshape(4, 4, 3))
    bsdf = ('<bsdf type="bumpmap"> <texture type="bitmap"> <string name="filename" value="b.pfm"/> <float name="gamma" value="1"/> </texture>'
            ' <bsdf type="coating"> <float name="intIOR" value="1.9"/> <bsdf type="diffuse"> <rgb name="reflectance" value="0.2, 0.5, 0.8"/> </bsdf> </bsdf> </bsdf>')
    body = '<shape type="obj"> <string name="filename" value="quad_vt.obj"/> %s </shape>' % bsdf
    desc, info = _load(tmp_path, body)
    assert not info["warnings"]
    m = desc.materials[-1]
    assert m["type"] == 0 and m["bump"] == 0 and m["coating"]["kind"] == "coating" and m["coating"]["eta"] == float(f32(1.9 / 1.000277))
    # the C++ loader reads no bitmaps: leniently it drops the bump map, and keeps the coat
    r, flat = _cpp(tmp_path, body, "--lenient")
    assert r.returncode == 0, r.stderr
    assert flat.endswith(_coat_bytes(desc)[-64:])


def test_scene_file_round_trip_and_old_files(tmp_path):
    desc = ppg_host.cbox_scene(8, 8)
    sl = np.stack([rtrans_slice("beckmann", 0.2, 1.49), rtrans_slice("ggx", 0.1, 1.5)])
    desc.rtrans = sl
    desc.materials = list(desc.materials) + [dict(DIFFUSE, coating=dict(SMOOTH_COAT)),
                                             dict({k: v for k, v in ROUGHPLASTIC.items() if k != "slice"}, rtrans=0, twosided=True,
                                                  coating=dict({k: v for k, v in ROUGH_COATS["ggx"].items() if k != "slice"}, slice=1, sample_visible=False))]
    p = str(tmp_path / "a.ppgs")
    ppg_host.save_scene(desc, p)
    back = ppg_host.load_scene_file(p)
    assert _coat_bytes(back) == _coat_bytes(desc) and back.materials[-1]["coating"]["slice"] == 1 and "coating" not in back.materials[0]
    q = str(tmp_path / "b.ppgs")
    ppg_host.save_scene(back, q)
    assert open(p, "rb").read() == open(q, "rb").read()
    # a file from before the block (the committed golden scene) still loads, and a scene without a coat writes no block
    old = ppg_host.load_scene_file(os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs"))
    assert not any("coating" in m for m in old.materials)
    ppg_host.save_scene(old, q)
    assert not int(np.frombuffer(open(q, "rb").read(), np.uint32, 6, 4)[5]) & 4096


REFUSED = {
    "coating(coating)": ('<bsdf type="coating"> <bsdf type="coating"> <bsdf type="diffuse"/> </bsdf> </bsdf>', "coating(coating) is not supported"),
    "coating(twosided)": ('<bsdf type="coating"> <bsdf type="twosided"> <bsdf type="diffuse"/> </bsdf> </bsdf>', "coating(twosided) is not supported"),
    "coating(mask)": ('<bsdf type="roughcoating"> <bsdf type="mask"> <bsdf type="diffuse"/> </bsdf> </bsdf>', "roughcoating(mask) is not supported"),
    "coating(bumpmap)": ('<bsdf type="coating"> <bsdf type="bumpmap"> <bsdf type="diffuse"/> </bsdf> </bsdf>', "coating(bumpmap) is not supported"),
    "no-nested": ('<bsdf type="coating"> <float name="intIOR" value="1.5"/> </bsdf>', "exactly one nested bsdf is required (found 0)"),
    "two-nested": ('<bsdf type="coating"> <bsdf type="diffuse"/> <bsdf type="diffuse"/> </bsdf>', "exactly one nested bsdf is required (found 2)"),
    "dielectric": ('<bsdf type="coating"> <bsdf type="dielectric"/> </bsdf>', "a coat on dielectric, thindielectric or roughdielectric is not supported"),
    "thindielectric": ('<bsdf type="roughcoating"> <bsdf type="thindielectric"/> </bsdf>', "a coat on dielectric, thindielectric or roughdielectric is not supported"),
    "roughdielectric": ('<bsdf type="coating"> <bsdf type="roughdielectric"/> </bsdf>', "a coat on dielectric, thindielectric or roughdielectric is not supported"),
    "roughcoating-conductor": ('<bsdf type="roughcoating"> <bsdf type="conductor"> %s </bsdf> </bsdf>' % NONE, "a roughcoating over a BSDF with a delta component"),
    "roughcoating-plastic": ('<bsdf type="roughcoating"> <bsdf type="plastic"/> </bsdf>', "a roughcoating over a BSDF with a delta component"),
    "texture-sigmaA": ('<bsdf type="coating"> <texture name="sigmaA" type="bitmap"> <string name="filename" value="t.pfm"/> </texture> <bsdf type="diffuse"/> </bsdf>',
                       "a texture on 'sigmaA' is not supported"),
    "texture-specular": ('<bsdf type="coating"> <texture name="specularReflectance" type="checkerboard"/> <bsdf type="diffuse"/> </bsdf>',
                         "a texture on 'specularReflectance' is not supported"),
    "texture-alpha": ('<bsdf type="roughcoating"> <texture name="alpha" type="bitmap"> <string name="filename" value="t.pfm"/> </texture> <bsdf type="diffuse"/> </bsdf>',
                      "a texture on 'alpha' is not supported"),
    "equal-iors": ('<bsdf type="coating"> <float name="intIOR" value="1.3"/> <float name="extIOR" value="1.3"/> <bsdf type="diffuse"/> </bsdf>',
                   "The interior and exterior indices of refraction must be positive and differ!"),
    "negative-ior": ('<bsdf type="coating"> <float name="intIOR" value="-1.5"/> <bsdf type="diffuse"/> </bsdf>',
                     "The interior and exterior indices of refraction must be positive and differ!"),
    "not-finite": ('<bsdf type="coating"> <float name="thickness" value="inf"/> <bsdf type="diffuse"/> </bsdf>', "a parameter is not finite"),
    "negative-thickness": ('<bsdf type="coating"> <float name="thickness" value="-1"/> <bsdf type="diffuse"/> </bsdf>', "thickness and sigmaA must not be negative"),
    "negative-sigmaA": ('<bsdf type="coating"> <rgb name="sigmaA" value="0.1, -0.2, 0"/> <bsdf type="diffuse"/> </bsdf>', "thickness and sigmaA must not be negative"),
    "aniso": ('<bsdf type="roughcoating"> <float name="alphaU" value="0.1"/> <float name="alphaV" value="0.2"/> <bsdf type="diffuse"/> </bsdf>',
              "The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_loaders_refuse_and_say_why(tmp_path, name):
    """strict loads refuse; lenient loads keep dropping such a coat around its nested BSDF, with a warning that says why"""
    bsdf, needle = REFUSED[name]
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, SPHERE % bsdf, data_dir=REF_DATA)
    assert needle in str(ei.value)
    r, _ = _cpp(tmp_path, SPHERE % bsdf, "--data-dir", REF_DATA)
    assert r.returncode != 0 and needle in r.stderr, r.stderr
    if name not in ("no-nested", "two-nested"):
        desc, info = _load(tmp_path, SPHERE % bsdf, strict=False, data_dir=REF_DATA)
        assert any("dropped around its nested bsdf" in w and needle in w for w in info["warnings"]), info["warnings"]
        # (of coating(coating(diffuse)) the inner coat is in order and stays)
        assert any("coating" in m for m in desc.materials) == (name == "coating(coating)")


def test_a_lenient_load_keeps_the_coat(tmp_path):
    bsdf = COAT_XML["coating-defaults-plastic"][0]
    desc, info = _load(tmp_path, SPHERE % bsdf + ' <shape type="sphere"> <bsdf type="ward"/> </shape>', strict=False)
    assert desc.materials[desc.spheres[0]["material"]]["coating"]["kind"] == "coating"
    assert not any("dropped" in w for w in info["warnings"]) and any("ward" in w for w in info["warnings"])
    r, flat = _cpp(tmp_path, SPHERE % bsdf, "--lenient")
    assert r.returncode == 0 and "dropped" not in r.stderr + r.stdout and int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 4096


def test_material_dicts():
    c = Coating.from_dict(dict(DIFFUSE, coating=dict(kind="roughcoating", eta=1.5, alpha=0.3, distribution="phong", slice=2, sigma_a=0.5)))
    assert (c.kind, c.distribution, c.sample_all, c.rtrans) == (2, 2, 0, 2) and list(c.sigma_a) == [0.5] * 3 and list(c.specular) == [1.0] * 3
    assert c.thickness == 1.0 and abs(c.alpha - 0.3) < 1e-7 and not any(c._reserved)
    assert bytes(Coating.from_dict(DIFFUSE)) == bytes(64) and Coating.from_dict(dict(kind=0)).kind == 0
    d = Coating.from_dict(dict(kind="coating"))
    assert d.kind == 1 and abs(d.eta - 1.5046 / 1.000277) < 1e-6  # bk7 / air
    assert Coating.from_dict(c.as_dict()).as_dict() == c.as_dict()
    import ctypes
    assert ctypes.sizeof(Coating) == 64
