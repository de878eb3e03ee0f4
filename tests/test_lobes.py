"""Mitsuba's `roughdiffuse`, `difftrans` and `phong` BSDFs (include/ppg.h PPG_BSDF_ROUGHDIFFUSE ..), on the CPU:

  * a numpy restatement of the three plug-ins in a precision of the caller's choice, written from their formulas — Oren-Nayar in its full
    and its qualitative form with sigma = alpha / sqrt(2); a cosine lobe on the far side of the surface; the modified Phong lobe
    (n + 2) / (2 pi) cos^n around the mirror direction plus a Lambertian term, chosen by the luminances — and checked on its own:
    densities that integrate to what they must, sample() against eval() and pdf(), a chi-square test of the sampled directions,
    reciprocity, the Lambertian limit, the albedo;
  * the same restatement run in float32 and in float64 over the items the GPU test (test_lobes_gpu.py) feeds the kernels: the figures
    that test derives its bounds from;
  * the hosts: material dicts, both scene loaders with BSDF::ensureEnergyConservation, the flat scene file, the oracle binding's refusal.

x^y is stated as exp(y log x), which is how the library computes it (include/ppg_detmath.h ppg_pow): in float32 that loses about
|y log x| 2^-24 of the value, which the float32 figures of the phong cases therefore carry.
"""
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import mitsuba_xml
from ppg_host.bindings import Material

from test_bsdfs import unit
from test_coatings import CHI2_SIGNIFICANCE, LUM, Sample, _hemisphere, _lattice_u, angle, cosine_hemisphere, rel
from test_microfacet_general import BIN, MESH_VT, SPHERE, WIS, _cpp, _material_records, _save, _scene

f32 = np.float32
EPSILON = 1e-4  # Mitsuba's Epsilon in single precision: the sines below it have no azimuth


# ------------------------------------------------------------------------------------------------ the restatement
def _pow(x, y, dt):
    """x^y for x >= 0 as exp(y log x), with the two cases that has no answer for: x^0 = 1 and 0^y = 0"""
    x = np.asarray(x, dt)
    y = np.asarray(y, dt)
    with np.errstate(all="ignore"):
        r = np.exp(y * np.log(x))
    return np.where(y == 0, dt(1), np.where(x == 0, dt(0), r)).astype(dt)


def _frame(n):
    """the tangents (s, t) of the frame Mitsuba builds around a unit vector n: t in the plane of n and its larger horizontal axis"""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    first = np.abs(x) > np.abs(y)
    with np.errstate(all="ignore"):
        ia, ib = 1 / np.sqrt(x * x + z * z), 1 / np.sqrt(y * y + z * z)
    zero = np.zeros_like(x)
    t = np.where(first[:, None], np.stack([z * ia, zero, -x * ia], 1), np.stack([zero, z * ib, -y * ib], 1))
    return np.cross(t, n), t


class Lobe:
    """one of the three BSDFs, with the two-sided adapter where the material asks for it; eval() is f |cos theta_o| in the solid-angle
    measure.  The parameters are the float32 values of the material record; `diffuse`: per-item values of the reflectance where a bitmap
    supplies it (the record then holds the bitmap's average, from which phong's sampling weight is still taken)."""

    def __init__(self, mat, dt=np.float64, diffuse=None):
        M = Material.from_dict(mat)
        self.dt, self.type = dt, int(M.type)
        assert self.type in (10, 11, 12)
        self.refl = np.asarray(list(M.reflectance), dt)[None] if diffuse is None else np.asarray(diffuse, f32).astype(dt)
        self.spec = np.asarray(list(M.specular), dt)[None]
        self.alpha = dt(M.alpha)  # roughdiffuse: alpha; phong: the exponent
        self.fast, self.twosided = bool(M.flags & 16), bool(M.flags & 1)
        lum = np.asarray(LUM, dt)
        d_avg, s_avg = (np.asarray(list(M.reflectance), dt) * lum).sum(), (np.asarray(list(M.specular), dt) * lum).sum()
        self.weight = dt(s_avg / (d_avg + s_avg)) if self.type == 12 else dt(0)

    # -- the one-sided plug-ins
    def _sines(self, wi, wo):
        dt = self.dt
        si = np.sqrt(np.maximum(dt(1) - wi[:, 2] * wi[:, 2], dt(0)))
        so = np.sqrt(np.maximum(dt(1) - wo[:, 2] * wo[:, 2], dt(0)))
        return si, so

    def _roughdiffuse(self, wi, wo):
        dt, one, inv_pi = self.dt, self.dt(1), self.dt(1 / np.pi)
        ci, co = wi[:, 2], wo[:, 2]
        sigma = self.alpha * (one / np.sqrt(dt(2)))
        s2 = sigma * sigma
        si, so = self._sines(wi, wo)
        with np.errstate(all="ignore"):
            cpd = (np.clip(wi[:, 0] / si, -1, 1) * np.clip(wo[:, 0] / so, -1, 1) + np.clip(wi[:, 1] / si, -1, 1) * np.clip(wo[:, 1] / so, -1, 1)).astype(dt)
            cpd = np.where((si > dt(EPSILON)) & (so > dt(EPSILON)), cpd, dt(0))
            first = ci > co
            sin_a, sin_b, tan_b = np.where(first, so, si), np.where(first, si, so), np.where(first, si / ci, so / co)
            if self.fast:
                A, B = one - dt(0.5) * s2 / (s2 + dt(0.33)), dt(0.45) * s2 / (s2 + dt(0.09))
                val = self.refl * (inv_pi * co * (A + B * np.maximum(cpd, dt(0)) * sin_a * tan_b))[:, None]
            else:
                ti, to = np.arccos(np.clip(ci, -1, 1)), np.arccos(np.clip(co, -1, 1))
                a, b = np.maximum(ti, to), np.minimum(ti, to)
                tmp, tmp2, tmp3 = s2 / (s2 + dt(0.09)), (dt(4) * inv_pi * inv_pi) * a * b, dt(2) * b * inv_pi
                C1 = one - dt(0.5) * s2 / (s2 + dt(0.33))
                C2 = dt(0.45) * tmp * np.where(cpd > 0, sin_a, sin_a - tmp3 * tmp3 * tmp3)
                C3, C4 = dt(0.125) * tmp * tmp2 * tmp2, dt(0.17) * s2 / (s2 + dt(0.13))
                tan_half = (sin_a + sin_b) / (np.sqrt(np.maximum(one - sin_a * sin_a, dt(0))) + np.sqrt(np.maximum(one - sin_b * sin_b, dt(0))))
                single = self.refl * (C1 + cpd * C2 * tan_b + (one - np.abs(cpd)) * C3 * tan_half)[:, None]
                double = self.refl * self.refl * (C4 * (one - cpd * tmp3 * tmp3))[:, None]
                val = (single + double) * (inv_pi * co)[:, None]
        return np.where(((ci > 0) & (co > 0))[:, None], val, dt(0)).astype(dt)

    def _lobe_cos(self, wi, wo):  # the cosine between wo and the mirror direction of wi
        return wo[:, 2] * wi[:, 2] - wo[:, 0] * wi[:, 0] - wo[:, 1] * wi[:, 1]

    def _phong(self, wi, wo):
        dt, n = self.dt, self.alpha
        ca = self._lobe_cos(wi, wo)
        glossy = np.where(ca > 0, (n + dt(2)) * dt(0.5 / np.pi) * _pow(np.maximum(ca, dt(0)), n, dt), dt(0))
        val = (self.spec * glossy[:, None] + self.refl * dt(1 / np.pi)) * wo[:, 2:3]
        return np.where(((wi[:, 2] > 0) & (wo[:, 2] > 0))[:, None], val, dt(0)).astype(dt)

    def _phong_pdf(self, wi, wo):
        dt, n = self.dt, self.alpha
        ca = self._lobe_cos(wi, wo)
        glossy = np.where(ca > 0, _pow(np.maximum(ca, dt(0)), n, dt) * (n + dt(1)) / dt(2 * np.pi), dt(0))
        p = self.weight * glossy + (dt(1) - self.weight) * (dt(1 / np.pi) * wo[:, 2])
        return np.where((wi[:, 2] > 0) & (wo[:, 2] > 0), p, dt(0)).astype(dt)

    def _eval_one(self, wi, wo):
        dt = self.dt
        if self.type == 10:
            return self._roughdiffuse(wi, wo)
        if self.type == 11:
            return np.where((wi[:, 2] * wo[:, 2] < 0)[:, None], self.refl * (dt(1 / np.pi) * np.abs(wo[:, 2]))[:, None], dt(0)).astype(dt)
        return self._phong(wi, wo)

    def _pdf_one(self, wi, wo):
        dt = self.dt
        if self.type == 10:
            return np.where((wi[:, 2] > 0) & (wo[:, 2] > 0), dt(1 / np.pi) * wo[:, 2], dt(0)).astype(dt)
        if self.type == 11:
            return np.where(wi[:, 2] * wo[:, 2] < 0, np.abs(wo[:, 2]) * dt(1 / np.pi), dt(0)).astype(dt)
        return self._phong_pdf(wi, wo)

    # -- with the two-sided adapter
    def _args(self, wi, wo=None):
        dt = self.dt
        wi = np.array(np.broadcast_to(np.asarray(wi, dt).reshape(-1, 3), (len(wo) if wo is not None else len(np.asarray(wi).reshape(-1, 3)), 3)))
        flip = (wi[:, 2] <= 0) & self.twosided
        wi[flip, 2] *= -1
        if wo is None:
            return wi, flip
        wo = np.array(np.asarray(wo, dt).reshape(-1, 3))
        wo[flip, 2] *= -1
        return wi, wo

    def eval(self, wi, wo):
        return self._eval_one(*self._args(wi, wo))

    def pdf(self, wi, wo):
        return self._pdf_one(*self._args(wi, wo))

    def eval_margin(self, wi, wo):
        """distance of an item of eval() / pdf() to the nearest branch point: the sine thresholds of roughdiffuse's azimuth"""
        if self.type != 10:
            return np.full(len(np.asarray(wo).reshape(-1, 3)), np.inf)
        si, so = self._sines(*self._args(wi, wo))
        return np.minimum(np.abs(si - EPSILON), np.abs(so - EPSILON))

    def sample(self, wi, u):
        dt = self.dt
        u = np.asarray(u, dt).reshape(-1, 2)
        wi = np.broadcast_to(np.asarray(wi, dt).reshape(-1, 3), (len(u), 3))
        wi, flipped = self._args(wi)
        n = len(u)
        margin = np.full(n, np.inf)
        if self.type == 11:
            wo = cosine_hemisphere(u, dt)
            wo[:, 2] = np.where(wi[:, 2] > 0, -wo[:, 2], wo[:, 2])
            pdf, w = np.abs(wo[:, 2]) * dt(1 / np.pi), np.broadcast_to(self.refl, (n, 3)).astype(dt)
        elif self.type == 10:
            wo = cosine_hemisphere(u, dt)
            pdf = dt(1 / np.pi) * wo[:, 2]
            w = self._roughdiffuse(wi, wo) / pdf[:, None]
            w = np.where((wi[:, 2] > 0)[:, None], w, dt(0))
            margin = self.eval_margin(wi, wo)
        else:
            ws = self.weight
            glossy = u[:, 0] <= ws
            margin = np.abs(u[:, 0].astype(np.float64) - float(ws))
            with np.errstate(all="ignore"):
                ux = np.where(glossy, u[:, 0] / ws, (u[:, 0] - ws) / (dt(1) - ws))
            e = self.alpha
            sin_a = np.sqrt(np.maximum(dt(1) - _pow(u[:, 1], dt(2) / (e + dt(1)), dt), dt(0)))
            cos_a = _pow(u[:, 1], dt(1) / (e + dt(1)), dt)
            phi = dt(2 * np.pi) * ux
            R = wi * np.asarray([-1, -1, 1], dt)[None]
            s, t = _frame(R)
            lobe = s * (sin_a * np.cos(phi))[:, None] + t * (sin_a * np.sin(phi))[:, None] + R * cos_a[:, None]
            wo = np.where(glossy[:, None], lobe, cosine_hemisphere(np.stack([ux, u[:, 1]], 1), dt)).astype(dt)
            margin = np.where(glossy, np.minimum(margin, np.abs(wo[:, 2])), margin)  # a rotated direction near the horizon
            pdf = self._phong_pdf(wi, wo)
            with np.errstate(all="ignore"):
                w = self._phong(wi, wo) / pdf[:, None]
            bad = (wi[:, 2] <= 0) | (glossy & (wo[:, 2] <= 0)) | (pdf == 0)
            w, pdf = np.where(bad[:, None], dt(0), w), np.where(bad, dt(0), pdf)
        out = Sample(wo.astype(dt), pdf.astype(dt), w.astype(dt), np.zeros(n, bool), margin).cleaned(dt)
        out.wo = np.where((flipped & out.weight.any(1))[:, None], out.wo * np.asarray([1, 1, -1], dt)[None], out.wo)
        return out


ROUGH = dict(type="roughdiffuse", reflectance=(0.2, 0.5, 0.8), alpha=0.5)
SHEET = dict(type="difftrans", reflectance=(0.6, 0.4, 0.2))
PHONG = dict(type="phong", reflectance=(0.5, 0.3, 0.2), specular=(0.2, 0.3, 0.4), exponent=30.0)
MODELS = dict(roughdiffuse=ROUGH, roughdiffuse_fast=dict(ROUGH, fast_approx=True), difftrans=SHEET, phong=PHONG, phong_wide=dict(PHONG, exponent=0.5))


def _sphere(n_theta, n_phi):
    th = (np.arange(n_theta) + 0.5) / n_theta * np.pi
    ph = (np.arange(n_phi) + 0.5) / n_phi * 2 * np.pi
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(TH) * np.cos(PH), np.sin(TH) * np.sin(PH), np.cos(TH)], -1).reshape(-1, 3)
    return d, (np.sin(TH) * (np.pi / n_theta) * (2 * np.pi / n_phi)).reshape(-1)


# ------------------------------------------------------------------------------------------------ 1. the restatement, checked on its own
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("wname", ["normal", "oblique", "grazing"])
def test_pdf_integrates_over_the_sphere(name, wname):
    """to 1 for the two cosine-sampled models; for phong to w_s (the lobe's mass above the horizon) + (1 - w_s), the mass taken in the
    lobe's OWN polar coordinates — (n + 1) / (2 pi) cos^n is normalised there in closed form — so that the two integrals share nothing
    but the lobe.  The quadratures' errors are what halving their steps shows."""
    b = Lobe(MODELS[name])
    wi = unit(WIS[wname]).astype(np.float64)[None]
    totals = []
    for n in (700, 1400):
        d, dw = _sphere(n, n)
        totals.append(float((b.pdf(wi, d) * dw).sum()))
    err = abs(totals[1] - totals[0])
    want = 1.0
    if b.type == 12:
        masses = []
        for n in (700, 1400):
            d, dw = _hemisphere(n, n)  # around the mirror direction R
            R = wi * [[-1, -1, 1]]
            s, t = _frame(R)
            world_z = d[:, 0] * s[0, 2] + d[:, 1] * t[0, 2] + d[:, 2] * R[0, 2]
            e = float(b.alpha)
            masses.append(float((((e + 1) / (2 * np.pi) * d[:, 2] ** e * dw)[world_z > 0]).sum()))
        err += abs(masses[1] - masses[0])
        want = float(b.weight) * masses[1] + 1 - float(b.weight)
        if wname == "normal":
            assert abs(masses[1] - 1) < 1e-5  # the whole lobe is above the horizon
    print(name, wname, "integral", totals, "expected", want, "quadrature error", err)
    assert err < 2e-3
    assert abs(totals[1] - want) <= 2 * err + 1e-9


@pytest.mark.parametrize("name,twosided", [(n, ts) for n in MODELS for ts in (False, True) if not (ts and n == "difftrans")])  # (a transmitter has no two-sided form)
@pytest.mark.parametrize("wname", list(WIS))
def test_sample_is_consistent_with_eval_and_pdf(name, twosided, wname):
    b = Lobe(dict(MODELS[name], twosided=twosided))
    wi = unit(WIS[wname]).astype(np.float64)
    s = b.sample(wi, _lattice_u(64))
    ok = s.weight.any(1)
    assert ok.any() == (wi[2] > 0 or twosided or b.type == 11)
    assert not s.delta.any()
    if not ok.any():
        return
    f, p = b.eval(wi, s.wo[ok]), b.pdf(wi, s.wo[ok])
    assert np.all(p > 0)
    assert np.allclose(s.pdf[ok], p, rtol=1e-12, atol=0)
    assert np.allclose(s.weight[ok] * s.pdf[ok][:, None], f, rtol=1e-12, atol=1e-300)
    side = np.sign(s.wo[ok][:, 2]) * np.sign(wi[2])
    assert np.all(side == (-1 if b.type == 11 else 1))
    if b.type == 11:  # rejection-free, and the weight is the transmittance itself
        assert ok.all() and np.array_equal(s.weight, np.broadcast_to(b.refl, s.weight.shape))


@pytest.mark.parametrize("name", list(MODELS))
def test_sampled_directions_follow_the_pdf(name):
    """test_chisquare.cpp's check as tests/test_coatings.py runs it, over the whole sphere: a histogram of sampled directions against the
    integral of pdf() per bin, Pearson's chi-square at the reference's significance level, bins expecting fewer than 5 pooled"""
    from scipy import stats
    b = Lobe(MODELS[name])
    wi = unit(WIS["oblique"]).astype(np.float64)
    n = 200000
    s = b.sample(wi, np.random.RandomState(3).rand(n, 2))
    sm = s.weight.any(1)
    nb_t, nb_p, sub = 20, 20, 16
    d, dw = _sphere(nb_t * sub, nb_p * sub)
    expect = (b.pdf(wi, d) * dw).reshape(nb_t, sub, nb_p, sub).sum((1, 3)) * n
    w = s.wo[sm]
    it = np.clip((np.arccos(np.clip(w[:, 2], -1, 1)) / np.pi * nb_t).astype(int), 0, nb_t - 1)
    ip = np.clip(((np.arctan2(w[:, 1], w[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nb_p).astype(int), 0, nb_p - 1)
    obs = np.zeros((nb_t, nb_p))
    np.add.at(obs, (it, ip), 1)
    obs, expect = np.append(obs.ravel(), n - sm.sum()), np.append(expect.ravel(), max(n - expect.sum(), 0.0))  # failed samples: one more cell
    order = np.argsort(expect)
    obs, expect = obs[order], expect[order]
    pooled = np.cumsum(expect) < 5
    o = np.append(obs[~pooled], obs[pooled].sum()) if pooled.any() else obs
    e = np.append(expect[~pooled], expect[pooled].sum()) if pooled.any() else expect
    keep = e > 0
    chi2 = float((((o - e) ** 2)[keep] / e[keep]).sum())
    p = float(stats.chi2.sf(chi2, int(keep.sum()) - 1))
    print(name, "chi2", chi2, "dof", int(keep.sum()) - 1, "p", p)
    assert p >= CHI2_SIGNIFICANCE


def _pairs(n=500, seed=5):
    rng = np.random.RandomState(seed)
    a = rng.randn(n, 3); a[:, 2] = np.abs(a[:, 2]) + 0.1; a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.randn(n, 3); b[:, 2] = np.abs(b[:, 2]) + 0.1; b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b


@pytest.mark.parametrize("exponent", [0.0, 0.5, 30.0, 400.0])
def test_phong_is_reciprocal(exponent):
    a, c = _pairs()
    b = Lobe(dict(PHONG, exponent=exponent))
    assert np.allclose(b.eval(a, c) / c[:, 2:3], b.eval(c, a) / a[:, 2:3], rtol=1e-12, atol=0)


@pytest.mark.parametrize("fast", [False, True])
def test_roughdiffuse_without_roughness_is_lambert(fast):
    a, c = _pairs()
    b = Lobe(dict(ROUGH, alpha=0.0, fast_approx=fast))
    assert np.allclose(b.eval(a, c), b.refl * (c[:, 2:3] / np.pi), rtol=1e-15, atol=0)
    s = b.sample(a, _lattice_u(23)[:len(a)])
    assert np.allclose(s.weight, np.broadcast_to(b.refl, s.weight.shape), rtol=1e-14, atol=0)


ALBEDO_CASES = [dict(ROUGH, reflectance=0.8, alpha=a, fast_approx=f) for a in (0.2, 0.7) for f in (False, True)] + [
    dict(SHEET, reflectance=1.0), dict(PHONG, reflectance=0.6, specular=0.4, exponent=0.0), dict(PHONG, reflectance=0.6, specular=0.4),
    dict(PHONG, reflectance=0.0, specular=1.0, exponent=400.0)]


@pytest.mark.parametrize("k", range(len(ALBEDO_CASES)))
@pytest.mark.parametrize("wname", ["normal", "oblique", "grazing"])
def test_the_albedo_stays_at_or_below_one(k, wname):
    """difftrans and phong with their parameters at the edge of what ensureEnergyConservation admits (a maximum, or a sum, of 1): a cosine
    lobe integrates to 1, and (n + 2) / (2 pi) cos^n cos theta_o to at most 1 (to 1 at normal incidence as n grows).  Oren and Nayar's
    model is NOT energy conserving at that edge — its interreflection term adds rho^2 C4 on top of a single-scattering term that already
    reaches the Lambertian's value: a white surface of alpha 0.2 returns 1.018 at the grazing direction used here (printed below for the
    white twin of each case) — so roughdiffuse is held at a reflectance of 0.8, the largest of the hook cases' channels."""
    if ALBEDO_CASES[k]["type"] == "roughdiffuse":
        white = Lobe(dict(ALBEDO_CASES[k], reflectance=1.0))
        d, dw = _sphere(500, 500)
        print("white twin:", float((white.eval(unit(WIS[wname]).astype(np.float64)[None], d)[:, 0] * dw).sum()))
    b = Lobe(ALBEDO_CASES[k])
    wi = unit(WIS[wname]).astype(np.float64)[None]
    totals = []
    for n in (500, 1000):
        d, dw = _sphere(n, n)
        totals.append((b.eval(wi, d) * dw[:, None]).sum(0))
    err = float(np.abs(totals[1] - totals[0]).max())
    print(ALBEDO_CASES[k], wname, "albedo", totals[1], "quadrature error", err)
    assert np.all(totals[1] > 0)
    assert np.all(totals[1] <= 1 + 2 * err + 1e-9)


# ------------------------------------------------------------------------------------------------ 2. float32 against float64
N = 500
MARGIN = 1e-4        # an item closer than this to a branch point is left out of the comparison ...
MAX_EXCLUDED = 0.01  # ... and no case may lose more than this share of its items
VALUE_FLOOR = 1e-2   # deviations of eval / pdf / weight are relative to max(|reference|, VALUE_FLOOR) (test_coatings.rel)
TEXELS = np.array([[[0.1, 0.2, 0.3], [0.8, 0.1, 0.1]], [[0.2, 0.7, 0.2], [0.5, 0.5, 0.6]]], f32)  # the 2 x 2 bitmap of the textured case

CASES = {}
for _a in (0.2, 0.7):
    for _fast in (True, False):
        for _ts in (False, True):
            CASES["roughdiffuse-%g-%s%s" % (_a, "fast" if _fast else "full", "-twosided" if _ts else "")] = dict(ROUGH, alpha=_a, fast_approx=_fast, twosided=_ts)
CASES["difftrans"] = dict(SHEET)
for _n in (0.5, 30.0, 400.0):
    for _d, _s in ((0.5, 0.2), (0.0, 0.6), (0.6, 0.0)):
        CASES["phong-%g-%g-%g" % (_n, _d, _s)] = dict(type="phong", exponent=_n, reflectance=(_d, 0.8 * _d, 0.6 * _d), specular=(_s, 0.9 * _s, 0.7 * _s))
CASES["phong-twosided"] = dict(PHONG, twosided=True)
CASES["phong-bitmap"] = dict(type="phong", exponent=30.0, specular=(0.2, 0.2, 0.3), texture=0,
                             reflectance=tuple(float(v) for v in TEXELS.reshape(-1, 3).mean(0, dtype=np.float64)))


def items(name):
    """500 items of a case from a generator seeded by its place in CASES: |cos theta| of wi and wo uniform in [0.02, 1], uniform azimuths,
    uniform sample points; half the wi below the surface for the two-sided cases and for difftrans, wo on either side for every case; for
    the textured case, uv at the centre of one of the bitmap's four texels (where bilinear interpolation returns the texel itself)."""
    m = CASES[name]
    rng = np.random.RandomState(100 + list(CASES).index(name))

    def direction(below):
        c = (0.02 + 0.98 * rng.rand(N)) * np.where(below, -1.0, 1.0)
        ph = 2 * np.pi * rng.rand(N)
        return np.stack([np.sqrt(1 - c * c) * np.cos(ph), np.sqrt(1 - c * c) * np.sin(ph), c], 1).astype(f32)
    both = bool(m.get("twosided")) or m["type"] == "difftrans"
    wi = direction((np.arange(N) % 2 == 1) if both else np.zeros(N, bool))
    wo = direction(rng.rand(N) < (0.5 if both else 0.2))
    u = rng.rand(N, 2).astype(f32)
    cell = rng.randint(0, 4, N)
    uv = np.stack([(cell % 2 + 0.5) / 2, (cell // 2 + 0.5) / 2], 1).astype(f32)
    return wi, wo, u, uv, (TEXELS[cell // 2, cell % 2] if "texture" in m else None)


def lobe_of(name, dt=np.float64):
    m = CASES[name]
    return Lobe({k: v for k, v in m.items() if k != "texture"}, dt, items(name)[4])


def reference(name):
    wi, wo, u, _, _ = items(name)
    b = lobe_of(name)
    s = b.sample(wi, u)
    return dict(eval=b.eval(wi, wo), pdf=b.pdf(wi, wo), sample=s, keep=s.margin >= MARGIN, keep_eval=b.eval_margin(wi, wo) >= MARGIN)


def deviations(got, ref):
    """largest deviation of eval, pdf, weight, sampled density and direction from the float64 reference, over the kept items (the sample's:
    those on which both sides produced one)"""
    ke, s, g = ref["keep_eval"], ref["sample"], got["sample"]
    both = ref["keep"] & s.weight.any(1) & np.asarray(g.weight).any(1)
    return dict(eval=float(rel(got["eval"], ref["eval"])[ke].max()), pdf=float(rel(got["pdf"], ref["pdf"])[ke].max()),
                weight=float(rel(np.asarray(g.weight)[both], s.weight[both]).max()) if both.any() else 0.0,
                sampled_pdf=float(rel(np.asarray(g.pdf)[both], s.pdf[both]).max()) if both.any() else 0.0,
                direction=float(angle(np.asarray(g.wo)[both], s.wo[both]).max()) if both.any() else 0.0)


_f32_cache = {}


def float32_figures(name):
    """(deviations of the float32 restatement from the float64 one, share of items excluded, share of kept items on which the two precisions
    disagree about whether there is a sample)"""
    if name not in _f32_cache:
        wi, wo, u, _, _ = items(name)
        b = lobe_of(name, f32)
        got = dict(eval=b.eval(wi, wo), pdf=b.pdf(wi, wo), sample=b.sample(wi, u))
        assert got["eval"].dtype == f32 and got["sample"].wo.dtype == f32
        ref = reference(name)
        keep = ref["keep"]
        differ = keep & (ref["sample"].weight.any(1) != got["sample"].weight.any(1))
        _f32_cache[name] = (deviations(got, ref), float(1 - (keep & ref["keep_eval"]).mean()), float(differ.sum() / max(1, keep.sum())))
    return _f32_cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_float32_restatement_against_float64(name):
    """The figures the GPU test's bounds come from.  Outside the exclusion rule the two precisions take the same branches, and the rule
    costs a case at most 1 % of its items (about 2e-4 of uniform sample points fall within the margin of phong's lobe choice)."""
    dev, excluded, differ = float32_figures(name)
    print(name, "float32 vs float64:", dev, "excluded", excluded, "different branches among the kept", differ)
    assert excluded <= MAX_EXCLUDED
    assert differ == 0
    assert all(np.isfinite(v) for v in dev.values())
    wi, wo, _, _, _ = items(name)
    assert np.abs(wi[:, 2]).min() >= 0.0199 and np.abs(wo[:, 2]).min() >= 0.0199 and (np.abs(wi[:, 2]) < 0.1).any()
    assert (wi[:, 2] < 0).any() == (bool(CASES[name].get("twosided")) or name == "difftrans")
    if name == "difftrans":  # the constant weight has no rounding at all
        assert dev["weight"] == 0


def test_the_edge_cases_of_pow():
    """sample.y = 0 puts the lobe direction on its equator (cos = 0, sin = 1); an exponent of 0 is the uniform lobe"""
    for dt in (np.float64, f32):
        assert _pow(np.zeros(1, dt), 1 / 31.0, dt)[0] == 0 and _pow(np.asarray([0.0, 0.3], dt), 0.0, dt).tolist() == [1, 1]
        b = Lobe(PHONG, dt)
        s = b.sample(unit(WIS["normal"]), np.asarray([[0.1, 0.0]], dt))
        assert s.wo[0, 2] == 0 and not s.weight.any()  # on the horizon: a failed sample
        b0 = Lobe(dict(PHONG, exponent=0.0), dt)
        wi, wo = unit(WIS["oblique"])[None], unit((0.1, 0.5, 0.7))[None]
        assert np.allclose(b0.pdf(wi, wo), float(b0.weight) / (2 * np.pi) + (1 - float(b0.weight)) * wo[0, 2] / np.pi, rtol=1e-6)
        assert np.isfinite(b0.sample(wi, np.asarray([[0.05, 0.0], [0.05, 0.5]], dt)).weight).all()


# ------------------------------------------------------------------------------------------------ 3. the hosts
def test_material_dicts():
    m = Material.from_dict(dict(type="roughdiffuse"))
    assert (m.type, m.flags) == (10, 0) and abs(m.alpha - 0.2) < 1e-7 and list(m.reflectance) == [0.5] * 3
    m = Material.from_dict(dict(type="roughdiffuse", alpha=0.0, fast_approx=True, twosided=True, opacity=0.25))
    assert (m.type, m.flags, m.alpha) == (10, 16 | 1 | 4, 0.0)
    m = Material.from_dict(dict(type="difftrans", reflectance=(0.1, 0.2, 0.3)))
    assert (m.type, m.flags) == (11, 0) and np.allclose(list(m.reflectance), (0.1, 0.2, 0.3))
    m = Material.from_dict(dict(type="phong"))
    assert m.type == 12 and m.alpha == 30.0 and np.allclose(list(m.specular), 0.2) and list(m.reflectance) == [0.5] * 3
    assert Material.from_dict(dict(type=12, exponent=7.5)).alpha == 7.5 and Material.from_dict(dict(type=12, alpha=7.5)).alpha == 7.5
    assert Material.from_dict(dict(type=0, fast_approx=False)).flags == 0
    assert Material.BSDF["phong"] == 12 and Material.LOBES == (10, 11, 12)


def test_oracle_binding_refuses_the_types(oracle_lib):
    from conftest import CBOX_PROPS, make_oracle
    for m in (ROUGH, SHEET, PHONG):
        desc = ppg_host.cbox_scene(16, 12)
        desc.materials = list(desc.materials) + [dict(m)]
        o = make_oracle(oracle_lib, **dict(CBOX_PROPS, budget=4))
        with pytest.raises(NotImplementedError) as err:
            o.set_scene(desc)
        assert "roughdiffuse, difftrans and phong are not implemented here" in str(err.value)


def test_scene_file_round_trip(tmp_path):
    """the flat file needs no new block: the types and the new flag bit travel in the ppg_material records, through both readers"""
    desc = ppg_host.cbox_scene(8, 8)
    desc.materials = list(desc.materials) + [dict(ROUGH, fast_approx=True, twosided=True), dict(SHEET, opacity=(0.5, 0.25, 1.0)), dict(PHONG)]
    want = b"".join(bytes(Material.from_dict(m)) for m in desc.materials)
    p = str(tmp_path / "a.ppgs")
    ppg_host.save_scene(desc, p)
    back = ppg_host.load_scene_file(p)
    assert b"".join(bytes(Material.from_dict(m)) for m in back.materials) == want
    assert back.materials[-3]["fast_approx"] is True and back.materials[-1]["type"] == 12 and "fast_approx" not in back.materials[-1]
    q = str(tmp_path / "b.ppgs")
    ppg_host.save_scene(back, q)
    assert open(p, "rb").read() == open(q, "rb").read()
    # the C++ reader and writer (ppg_render): the same records come out
    out = str(tmp_path / "c.ppgs")
    _cpp(tmp_path, SPHERE % '<bsdf type="diffuse"/>')  # (builds the C++ host where it is missing)
    r = subprocess.run([BIN, "--ppgs", out, "-q", p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _material_records(open(out, "rb").read()) == want


def _records(desc):
    return b"".join(bytes(Material.from_dict(m)) for m in desc.materials)


def _load(tmp_path, body, **kw):
    desc, _, info = ppg_host.load_scene(_scene(tmp_path, body), **kw)
    return desc, info


S = 0.99 / 1.5  # the rescale of a maximum of 1.5
LOBE_XML = {  # name: (the <bsdf>, what the material dict must hold)
    "roughdiffuse-defaults": ('<bsdf type="roughdiffuse"/>', dict(type=10, reflectance=(0.5, 0.5, 0.5), alpha=float(f32(0.2)))),
    "difftrans-defaults": ('<bsdf type="difftrans"/>', dict(type=11, reflectance=(0.5, 0.5, 0.5))),
    "phong-defaults": ('<bsdf type="phong"/>', dict(type=12, reflectance=(0.5, 0.5, 0.5), specular=(float(f32(0.2)),) * 3, exponent=30.0)),
    "roughdiffuse-explicit": ('<bsdf type="roughdiffuse"> <rgb name="reflectance" value="0.25, 0.5, 0.75"/> <float name="alpha" value="0.7"/>'
                              ' <boolean name="useFastApprox" value="true"/> </bsdf>', dict(type=10, reflectance=(0.25, 0.5, 0.75), alpha=float(f32(0.7)), fast_approx=True)),
    "roughdiffuse-other-name": ('<bsdf type="roughdiffuse"> <rgb name="diffuseReflectance" value="0.25, 0.5, 0.75"/> <float name="alpha" value="0"/> </bsdf>',
                                dict(type=10, reflectance=(0.25, 0.5, 0.75), alpha=0.0)),
    "difftrans-explicit": ('<bsdf type="difftrans"> <rgb name="transmittance" value="0.5, 0.25, 0.125"/> </bsdf>', dict(type=11, reflectance=(0.5, 0.25, 0.125))),
    "phong-explicit": ('<bsdf type="phong"> <rgb name="diffuseReflectance" value="0.25, 0.5, 0.125"/> <rgb name="specularReflectance" value="0.5, 0.25, 0.125"/>'
                       ' <float name="exponent" value="400"/> </bsdf>', dict(type=12, reflectance=(0.25, 0.5, 0.125), specular=(0.5, 0.25, 0.125), exponent=400.0)),
    "mask-twosided-phong": ('<bsdf type="mask"> <rgb name="opacity" value="0.5, 0.25, 1"/> <bsdf type="twosided"> <bsdf type="phong"/> </bsdf> </bsdf>',
                            dict(type=12, twosided=True, opacity=(0.5, 0.25, 1.0))),
    "twosided-roughdiffuse": ('<bsdf type="twosided"> <bsdf type="roughdiffuse"/> </bsdf>', dict(type=10, twosided=True)),
    "mask-difftrans": ('<bsdf type="mask"> <bsdf type="difftrans"/> </bsdf>', dict(type=11, opacity=(0.5, 0.5, 0.5))),
    # BSDF::ensureEnergyConservation: one parameter above 1; a pair whose sum is; switched off
    "roughdiffuse-too-bright": ('<bsdf type="roughdiffuse"> <rgb name="reflectance" value="0.75, 1.5, 0.5"/> </bsdf>',
                                dict(type=10, reflectance=tuple(float(f32(v) * (f32(0.99) * (f32(1) / f32(1.5)))) for v in (0.75, 1.5, 0.5)))),
    "difftrans-too-bright": ('<bsdf type="difftrans"> <rgb name="transmittance" value="2, 2, 2"/> </bsdf>',
                             dict(type=11, reflectance=(float(f32(2) * (f32(0.99) * (f32(1) / f32(2)))),) * 3)),
    "phong-too-bright": ('<bsdf type="phong"> <rgb name="diffuseReflectance" value="0.75, 0.5, 0.25"/> <rgb name="specularReflectance" value="0.75, 0.25, 0.25"/> </bsdf>',
                         dict(type=12, reflectance=tuple(float(f32(v) * (f32(0.99) * (f32(1) / f32(1.5)))) for v in (0.75, 0.5, 0.25)),
                              specular=tuple(float(f32(v) * (f32(0.99) * (f32(1) / f32(1.5)))) for v in (0.75, 0.25, 0.25)))),
    "phong-bright-but-unchecked": ('<bsdf type="phong"> <rgb name="diffuseReflectance" value="0.75, 0.5, 0.25"/> <rgb name="specularReflectance" value="0.75, 0.25, 0.25"/>'
                                   ' <boolean name="ensureEnergyConservation" value="false"/> </bsdf>', dict(type=12, reflectance=(0.75, 0.5, 0.25), specular=(0.75, 0.25, 0.25))),
    "phong-sum-of-one": ('<bsdf type="phong"> <rgb name="diffuseReflectance" value="0.75, 0.5, 0.25"/> <rgb name="specularReflectance" value="0.25, 0.25, 0.25"/> </bsdf>',
                         dict(type=12, reflectance=(0.75, 0.5, 0.25), specular=(0.25, 0.25, 0.25))),
}


@pytest.mark.parametrize("name", list(LOBE_XML))
def test_both_loaders_read_the_plugins_and_agree(tmp_path, name):
    """the Python loader's dicts; the C++ loader (ppg_render --ppgs) writes the same ppg_material records, byte for byte; a rescale for
    energy conservation is announced by both"""
    bsdf, want = LOBE_XML[name]
    desc, info = _load(tmp_path, SPHERE % bsdf)
    m = desc.materials[desc.spheres[0]["material"]]
    for k, v in want.items():
        assert m[k] == v, (k, m)
    bright = "too-bright" in name
    assert len(info["warnings"]) == (1 if bright else 0), info["warnings"]
    r, flat = _cpp(tmp_path, SPHERE % bsdf)
    assert r.returncode == 0, r.stderr
    assert _material_records(flat) == _records(desc) == _material_records(open(_save(desc, tmp_path), "rb").read())
    if bright:
        assert "violates energy conservation" in info["warnings"][0] and "scaled by" in info["warnings"][0]
        loud = subprocess.run([BIN, "--ppgs", str(tmp_path / "x.ppgs"), _scene(tmp_path, SPHERE % bsdf)], capture_output=True, text=True)
        assert "violates energy conservation" in loud.stderr
    # ... and the XML writer gives the same records back (the values are final: it switches the check off)
    again, _, info2 = ppg_host.load_scene(ppg_host.save_scene_xml(desc, dict(budgetType="spp", budget=8.0), str(tmp_path / "w")))
    assert not info2["warnings"] and bytes(Material.from_dict(m)) in [bytes(Material.from_dict(x)) for x in again.materials]


def test_a_named_bsdf_is_referenced(tmp_path):
    body = ('<bsdf type="phong" id="shiny"> <float name="exponent" value="12"/> </bsdf> <bsdf type="difftrans" id="shade"/>'
            ' <shape type="sphere"> <ref id="shiny"/> </shape> <shape type="sphere"> <point name="center" x="3" y="0" z="0"/> <ref id="shade"/> </shape>')
    desc, info = _load(tmp_path, body)
    assert not info["warnings"]
    a, b = (desc.materials[s["material"]] for s in desc.spheres)
    assert (a["type"], a["exponent"], b["type"]) == (12, 12.0, 11)
    r, flat = _cpp(tmp_path, body)
    assert r.returncode == 0, r.stderr
    assert _material_records(flat) == _records(desc)


def _write_bitmap(tmp_path, rgb, name="t.pfm"):
    from ppg_host import imageio
    imageio.write_pfm(str(tmp_path / name), np.asarray(rgb, f32))


BITMAP = '<texture name="%s" type="bitmap"> <string name="filename" value="t.pfm"/> </texture>'


@pytest.mark.parametrize("plugin,param", [("roughdiffuse", "reflectance"), ("difftrans", "transmittance"), ("phong", "diffuseReflectance")])
def test_a_bitmap_on_the_reflectance(tmp_path, plugin, param):
    """inside bumpmap(mask(twosided(x))) where x can be two-sided: the record holds the bitmap's average, the texture word both indices"""
    _write_bitmap(tmp_path, TEXELS)
    _write_bitmap(tmp_path, np.linspace(0, 1, 48, dtype=f32).reshape(4, 4, 3), "b.pfm")
    leaf = '<bsdf type="%s"> %s </bsdf>' % (plugin, BITMAP % param)
    if plugin != "difftrans":
        leaf = '<bsdf type="twosided"> %s </bsdf>' % leaf
    bsdf = ('<bsdf type="bumpmap"> <texture type="bitmap"> <string name="filename" value="b.pfm"/> <float name="gamma" value="1"/> </texture>'
            ' <bsdf type="mask"> %s </bsdf> </bsdf>' % leaf)
    desc, info = _load(tmp_path, MESH_VT % bsdf)
    assert not info["warnings"]
    m = desc.materials[-1]
    assert m["type"] == Material.BSDF[plugin] and bool(m.get("twosided")) == (plugin != "difftrans") and m["opacity"] == (0.5, 0.5, 0.5)
    assert np.array_equal(desc.textures[m["texture"]]["rgb"], TEXELS) and desc.textures[m["bump"]]["rgb"].shape == (4, 4, 3)
    assert np.allclose(m["reflectance"], TEXELS.reshape(-1, 3).mean(0), rtol=1e-6)
    M = Material.from_dict(m)
    assert M.texture == (m["texture"] + 1) | ((m["bump"] + 1) << 16) and M.flags == (4 | (0 if plugin == "difftrans" else 1))
    # the C++ loader reads no bitmaps: leniently it keeps the plug-in with the parameter's default, inside the adapters it does read
    r, flat = _cpp(tmp_path, MESH_VT % bsdf, "--lenient")
    assert r.returncode == 0, r.stderr
    rec = Material.from_buffer_copy(_material_records(flat)[-80:])
    assert (rec.type, rec.flags, rec.texture) == (M.type, M.flags, 0) and list(rec.reflectance) == [0.5] * 3


def test_energy_conservation_takes_a_bitmaps_maximum(tmp_path):
    """single form: the maximum over the decoded texels; pair form: that maximum plus the constant.  The scaled bitmap is a texture of its
    own, and the record holds the scaled average."""
    tex = TEXELS * f32(1.5)  # maximum 1.2 (red of texel (0, 1))
    _write_bitmap(tmp_path, tex)
    peak = f32(tex.reshape(-1, 3).max(0).max())
    desc, info = _load(tmp_path, MESH_VT % ('<bsdf type="roughdiffuse"> %s </bsdf>' % (BITMAP % "reflectance")))
    scale = f32(0.99) * (f32(1) / peak)
    m = desc.materials[-1]
    assert len(info["warnings"]) == 1 and "violates energy conservation" in info["warnings"][0]
    assert np.array_equal(desc.textures[m["texture"]]["rgb"], tex * scale) and float(desc.textures[m["texture"]]["rgb"].max()) <= 0.99 + 1e-6
    assert np.allclose(m["reflectance"], tex.reshape(-1, 3).mean(0) * scale, rtol=1e-6)
    # phong: the bitmap alone stays below 1, with the specular constant the sum does not
    _write_bitmap(tmp_path, TEXELS)
    body = '<bsdf type="phong"> %s <rgb name="specularReflectance" value="0.5, 0.5, 0.5"/> </bsdf>' % (BITMAP % "diffuseReflectance")
    desc, info = _load(tmp_path, MESH_VT % body)
    total = f32((TEXELS.reshape(-1, 3).max(0) + f32(0.5)).max())
    scale = f32(0.99) * (f32(1) / total)
    m = desc.materials[-1]
    assert len(info["warnings"]) == 1 and '"specularReflectance" and "diffuseReflectance" sum to' in info["warnings"][0]
    assert m["specular"] == (float(f32(0.5) * scale),) * 3 and np.array_equal(desc.textures[m["texture"]]["rgb"], TEXELS * scale)
    desc, info = _load(tmp_path, MESH_VT % ('<bsdf type="phong"> %s <rgb name="specularReflectance" value="0.1, 0.1, 0.1"/> </bsdf>' % (BITMAP % "diffuseReflectance")))
    assert not info["warnings"] and np.array_equal(desc.textures[desc.materials[-1]["texture"]]["rgb"], TEXELS)


REFUSED = {
    "twosided(difftrans)": ('<bsdf type="twosided"> <bsdf type="difftrans"/> </bsdf>', "twosided(difftrans): only BRDFs can be two-sided"),
    "texture-alpha": ('<bsdf type="roughdiffuse"> %s </bsdf>' % (BITMAP % "alpha"), "roughdiffuse: a texture on 'alpha' is not supported"),
    "texture-exponent": ('<bsdf type="phong"> %s </bsdf>' % (BITMAP % "exponent"), "phong: a texture on 'exponent' is not supported"),
    "texture-specular": ('<bsdf type="phong"> %s </bsdf>' % (BITMAP % "specularReflectance"), "phong: a texture on 'specularReflectance' is not supported"),
    "coating(phong)": ('<bsdf type="coating"> <bsdf type="phong"/> </bsdf>', "a coat on roughdiffuse, difftrans or phong is not supported"),
    "blend(difftrans)": ('<bsdf type="blendbsdf"> <float name="weight" value="0.5"/> <bsdf type="diffuse"/> <bsdf type="difftrans"/> </bsdf>',
                         "roughdiffuse, difftrans and phong children are not supported"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_loaders_refuse_and_say_why(tmp_path, name):
    bsdf, needle = REFUSED[name]
    _write_bitmap(tmp_path, TEXELS)
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, MESH_VT % bsdf)
    assert needle in str(ei.value)
    r, _ = _cpp(tmp_path, MESH_VT % bsdf)
    assert r.returncode != 0 and needle in r.stderr, r.stderr


def test_the_types_that_stay_refused_say_which_are_read(tmp_path):
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, SPHERE % '<bsdf type="hk"/>')
    assert "is not supported yet (diffuse, roughdiffuse, difftrans, phong," in str(ei.value)
    r, _ = _cpp(tmp_path, SPHERE % '<bsdf type="hk"/>')
    assert r.returncode != 0 and "is not supported yet (diffuse, roughdiffuse, difftrans, phong," in r.stderr
