"""Mitsuba's `blendbsdf` and `mixturebsdf` combinators (include/ppg.h ppg_set_blends), on the CPU:

  * a numpy restatement of both plug-ins in a precision of the caller's choice, on the leaf restatement of test_coatings.py plus the
    discrete-measure eval / pdf of conductor and plastic, checked on its own: closed forms, sample() against the integral of eval(), a
    chi-square test of the sampled directions, the limits;
  * the lattice and the cases the GPU test (test_blends_gpu.py) feeds the kernels, run here in float32 and in float64: the figures that
    test derives its bounds from, and the exclusion mask with its cap;
  * the hosts: material dicts, the flat scene file, both scene loaders, the XML writer.
"""
import os

import numpy as np
import pytest

import ppg_host
from ppg_host import mitsuba_xml
from ppg_host.bindings import Blend, expand_blends, has_blends

from test_bsdfs import GOLD, unit
from test_coatings import (CHI2_SIGNIFICANCE, COPPER, DIFFUSE, MARGIN, MAX_EXCLUDED, PLASTIC, ROUGHPLASTIC, Leaf, Sample, _v, deviations, dot,
                           fresnel_conductor, fresnel_dielectric, lattice)
from test_microfacet_general import WIS, Distribution

f32 = np.float32
DELTA_EPSILON = 1e-3  # the tolerance of the plug-ins' mirror-direction test

LEAVES = dict(diffuse=DIFFUSE, gold=GOLD, copper=COPPER, plastic=PLASTIC, roughplastic=ROUGHPLASTIC)
SILVER = dict(type="conductor", eta=(0.155, 0.117, 0.138), k=(4.828, 3.122, 2.147), reflectance=(0.9, 1.0, 0.8))
ANISO_GOLD = dict(GOLD, alpha=0.1, alpha_v=0.3)  # a general microfacet entry (ppg_set_microfacet): alphaU != alphaV
# the two texels of the nearest-filtered bitmaps: a weight map (averages 0.3 and 0.7) and a reflectance map
TEXELS_W = np.array([[0.2, 0.3, 0.4], [0.6, 0.7, 0.8]], f32)
TEXELS_R = np.array([[0.2, 0.5, 0.8], [0.6, 0.3, 0.1]], f32)


# ------------------------------------------------------------------------------------------------ the restatement
def derived_weights(kind, weight=None, weights=None, ensure=True):
    """(eval weights, pdf probabilities, cdf) of a combinator with constant weights, as ppg_set_scene derives them: in float32"""
    if kind == "blendbsdf":
        w = min(f32(1), max(f32(0), f32(weight)))
        we = [f32(1) - w, w]
        return we, list(we), [f32(0), we[0], f32(1)]
    we = [f32(v) for v in weights]
    total = f32(0)
    for v in we:
        total = f32(total + v)
    assert total > 0
    if ensure and total > 1:
        scale = f32(1) / total
        we = [f32(v * scale) for v in we]
    cdf = [f32(0)]
    for v in we:
        cdf.append(f32(cdf[-1] + v))
    norm = f32(1) / cdf[-1]
    cdf = [cdf[0]] + [f32(c * norm) for c in cdf[1:]]
    cdf[-1] = f32(1)
    return we, [f32(cdf[i + 1] - cdf[i]) for i in range(len(we))], cdf


def mirror_error(wi, wo):
    return np.abs(dot(wi * np.asarray([-1, -1, 1], wi.dtype)[None], wo) - wi.dtype.type(1))


def leaf_eval_discrete(leaf, wi, wo):
    """eval() under the discrete measure: the delta component when wo is wi's mirror direction, nothing otherwise"""
    dt = leaf.dt
    wi, wo = _v(wi, dt), _v(wo, dt)
    ok = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    safe = np.where(ok[:, None], wi, np.asarray([0, 0, 1], dt)[None])
    with np.errstate(all="ignore"):
        if leaf.type == "conductor":
            ok = ok & ~(mirror_error(wi, wo) > dt(DELTA_EPSILON))
            r = leaf.refl[None] * fresnel_conductor(safe[:, 2], leaf.eta, leaf.k, dt)
        elif leaf.type == "plastic":
            ok = ok & (mirror_error(wi, wo) < dt(DELTA_EPSILON))
            r = leaf.spec[None] * fresnel_dielectric(safe[:, 2], leaf.eta, dt)[0][:, None]
        else:
            return np.zeros_like(wo)
    return np.where(ok[:, None], r, dt(0)).astype(dt)


def leaf_pdf_discrete(leaf, wi, wo):
    dt = leaf.dt
    wi, wo = _v(wi, dt), _v(wo, dt)
    ok = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    safe = np.where(ok[:, None], wi, np.asarray([0, 0, 1], dt)[None])
    with np.errstate(all="ignore"):
        if leaf.type == "conductor":
            ok = ok & ~(mirror_error(wi, wo) > dt(DELTA_EPSILON))
            r = np.ones(len(wo), dt)
        elif leaf.type == "plastic":
            ok = ok & (mirror_error(wi, wo) < dt(DELTA_EPSILON))
            r = leaf._ps(safe)
        else:
            return np.zeros(len(wo), dt)
    return np.where(ok, r, dt(0)).astype(dt)


def make_leaf(mat, dt):
    leaf = Leaf({k: v for k, v in mat.items() if k != "alpha_v"}, dt)
    if "alpha_v" in mat:  # the general entry: alphaU / alphaV with visible-normal sampling
        leaf.distr = Distribution(mat.get("distribution", "ggx"), f32(mat["alpha"]), f32(mat["alpha_v"]), dt)
    return leaf


class Mix:
    """`blendbsdf` (weights (1 - w, w), chosen by sample.x < 1 - w) or `mixturebsdf` (eval weights, chosen by the normalised
    distribution with the sample reused) over Leafs, optionally inside a two-sided adapter.  `weight` of a blend: a number, or the
    texel(s) of a weight map, [3] or [n, 3], of which it takes the clamped average."""

    def __init__(self, kind, children, weight=None, weights=None, ensure=True, twosided=False, dt=np.float64):
        self.dt, self.kind, self.twosided = dt, kind, twosided
        self.leaves = [c if isinstance(c, Leaf) else make_leaf(c, dt) for c in children]
        if kind == "blendbsdf":
            assert len(self.leaves) == 2
            if np.ndim(weight) == 0:
                w = np.asarray(derived_weights(kind, weight)[0][1], f32).astype(dt).reshape(1)
            else:
                t = np.asarray(weight, f32).astype(dt).reshape(-1, 3)
                avg = (((dt(0) + t[:, 0]) + t[:, 1]) + t[:, 2]) * (dt(1) / dt(3))
                w = np.minimum(dt(1), np.maximum(dt(0), avg))
            self.we = [dt(1) - w, w]
            self.wp = self.we
            self.cdf = [np.zeros_like(w), self.we[0], np.ones_like(w)]
        else:
            we, wp, cdf = derived_weights(kind, weights=weights, ensure=ensure)
            cast = lambda v: np.asarray(v, f32).astype(dt).reshape(1)  # noqa: E731
            self.we, self.cdf = [cast(v) for v in we], [cast(v) for v in cdf]
            self.wp = [self.cdf[i + 1] - self.cdf[i] for i in range(len(we))]

    def _local(self, wi, wo=None):
        dt = self.dt
        wi = _v(wi, dt).copy()
        wo = None if wo is None else np.broadcast_to(_v(wo, dt), (max(len(wi), len(_v(wo, dt))), 3)).copy()
        if wo is not None and len(wi) != len(wo):
            wi = np.broadcast_to(wi, wo.shape).copy()
        return wi, wo

    def eval(self, wi, wo):
        wi, wo = self._local(wi, wo)
        if self.twosided:
            f = ~(wi[:, 2] > 0)
            wi[f, 2] *= -1; wo[f, 2] *= -1
        r = np.zeros_like(wo)
        for leaf, we in zip(self.leaves, self.we):
            r = r + leaf.eval(wi, wo) * we[:, None]
        return r.astype(self.dt)

    def pdf(self, wi, wo):
        wi, wo = self._local(wi, wo)
        if self.twosided:
            f = ~(wi[:, 2] > 0)
            wi[f, 2] *= -1; wo[f, 2] *= -1
        r = np.zeros(len(wo), self.dt)
        for leaf, wp in zip(self.leaves, self.wp):
            r = r + leaf.pdf(wi, wo) * wp
        return r.astype(self.dt)

    def choose(self, u0):
        """(child, reused sample, distance of u0 to the nearest edge between two children that can be chosen)"""
        dt = self.dt
        n, k = len(u0), len(self.leaves)
        cdf = np.stack([np.broadcast_to(c, (n,)) for c in self.cdf], 1)  # [n, k + 1]
        if self.kind == "blendbsdf":
            entry = np.where(u0 < cdf[:, 1], 0, 1)
        else:  # DiscreteDistribution::sample: lower_bound, one back, clamped, then past entries of probability 0
            entry = np.clip((cdf < u0[:, None]).sum(1) - 1, 0, k - 1)
            for _ in range(k):
                width = np.take_along_axis(cdf, entry[:, None] + 1, 1)[:, 0] - np.take_along_axis(cdf, entry[:, None], 1)[:, 0]
                entry = np.where((width == 0) & (entry < k - 1), entry + 1, entry)
        c0 = np.take_along_axis(cdf, entry[:, None], 1)[:, 0]
        c1 = np.take_along_axis(cdf, entry[:, None] + 1, 1)[:, 0]
        with np.errstate(all="ignore"):
            reused = (u0 - c0) / (c1 - c0)
            if self.kind == "blendbsdf":  # (sample.x /= weights[0]: the same number)
                reused = np.where(entry == 0, u0 / cdf[:, 1], reused)
        inner = cdf[:, 1:-1].astype(np.float64)
        margin = np.abs(inner - u0[:, None].astype(np.float64)).min(1) if k > 1 else np.full(n, np.inf)
        return entry, reused.astype(dt), margin

    def sample(self, wi, u):
        dt = self.dt
        wi, _ = self._local(wi)
        u = np.asarray(u, dt).reshape(-1, 2)
        n = len(u)
        if len(wi) != n:
            wi = np.broadcast_to(wi, (n, 3)).copy()
        flipped = np.zeros(n, bool)
        if self.twosided:
            flipped = wi[:, 2] < 0
            wi[flipped, 2] *= -1
        entry, reused, margin = self.choose(u[:, 0])
        ur = np.stack([np.where(np.isfinite(reused), reused, dt(0.5)), u[:, 1]], 1)
        wo, pdf, weight = np.zeros((n, 3), dt), np.zeros(n, dt), np.zeros((n, 3), dt)
        delta = np.zeros(n, bool)
        for c, leaf in enumerate(self.leaves):
            s = leaf.sample(wi, ur)
            m = entry == c
            wo, pdf, weight = np.where(m[:, None], s.wo, wo), np.where(m, s.pdf, pdf), np.where(m[:, None], s.weight, weight)
            delta, margin = np.where(m, s.delta, delta), np.where(m, np.minimum(margin, s.margin), margin)
        ok = weight.any(1)
        bw = lambda ws: np.take_along_axis(np.stack([np.broadcast_to(w, (n,)) for w in ws], 1), entry[:, None], 1)[:, 0]  # noqa: E731
        with np.errstate(all="ignore"):
            result = weight * (bw(self.we) * pdf)[:, None]
            pdf = pdf * bw(self.wp)
            for c, leaf in enumerate(self.leaves):
                other = (entry != c)
                p = np.where(delta, leaf_pdf_discrete(leaf, wi, wo), leaf.pdf(wi, wo))
                f = np.where(delta[:, None], leaf_eval_discrete(leaf, wi, wo), leaf.eval(wi, wo))
                pdf = pdf + np.where(other, p * self.wp[c], dt(0))
                result = result + np.where(other[:, None], f * self.we[c][:, None], dt(0))
            weight = result / pdf[:, None]
            ok = ok & (pdf > 0) & np.isfinite(pdf)
        weight, pdf = np.where(ok[:, None], weight, dt(0)), np.where(ok, pdf, dt(0))
        wo = np.where(ok[:, None], wo, dt(0))
        wo = np.where((flipped & ok)[:, None], wo * np.asarray([1, 1, -1], dt)[None], wo)
        s = Sample(wo.astype(dt), pdf.astype(dt), weight.astype(dt), delta & ok, margin).cleaned(dt)
        s.entry = entry
        return s


# ------------------------------------------------------------------------------------------------ 1. the restatement on its own
def _pairs(n=400, seed=7):
    rng = np.random.RandomState(seed)
    a = rng.randn(n, 3); a[:, 2] = np.abs(a[:, 2]) + 0.1; a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.randn(n, 3); b[:, 2] = np.abs(b[:, 2]) + 0.1; b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b


def test_blend_of_two_diffuse_is_diffuse_of_the_mixed_reflectance():
    a, b = _pairs()
    d0, d1 = DIFFUSE, dict(type="diffuse", reflectance=(0.7, 0.1, 0.3))
    m = Mix("blendbsdf", [d0, d1], weight=0.3)
    w0, w1 = float(m.we[0][0]), float(m.we[1][0])
    mixed = np.asarray(d0["reflectance"], f32).astype(np.float64) * w0 + np.asarray(d1["reflectance"], f32).astype(np.float64) * w1
    want = Leaf(DIFFUSE).eval(a, b) / Leaf(DIFFUSE).refl[None] * mixed[None]
    assert np.allclose(m.eval(a, b), want, rtol=1e-13, atol=0)
    assert np.allclose(m.pdf(a, b), Leaf(DIFFUSE).pdf(a, b), rtol=1e-13, atol=0)
    s = m.sample(a, np.random.RandomState(1).rand(len(a), 2))
    assert np.allclose(s.weight, mixed[None], rtol=1e-12) and not s.delta.any()


def test_two_conductors_after_a_delta_sample():
    a, _ = _pairs()
    m = Mix("blendbsdf", [COPPER, SILVER], weight=0.3)
    s = m.sample(a, np.random.RandomState(2).rand(len(a), 2))
    f0 = Leaf(COPPER).refl[None] * fresnel_conductor(a[:, 2], Leaf(COPPER).eta, Leaf(COPPER).k, np.float64)
    f1 = Leaf(SILVER).refl[None] * fresnel_conductor(a[:, 2], Leaf(SILVER).eta, Leaf(SILVER).k, np.float64)
    w0, w1 = m.we[0][0], m.we[1][0]
    assert s.delta.all() and np.allclose(s.pdf, 1.0, rtol=1e-7)  # (w0 + w1 of the float32 weights)
    assert np.allclose(s.weight, (w0 * f0 + w1 * f1) / (w0 + w1), rtol=1e-12)
    assert np.allclose(s.wo, a * [-1, -1, 1]) and set(np.unique(s.entry)) == {0, 1}


def test_conductor_and_diffuse_after_a_delta_sample():
    a, _ = _pairs()
    m = Mix("blendbsdf", [COPPER, DIFFUSE], weight=0.3)
    s = m.sample(a, np.random.RandomState(3).rand(len(a), 2))
    d = s.delta
    assert d.any() and (~d).any() and np.array_equal(d, s.entry == 0)
    f0 = Leaf(COPPER).refl[None] * fresnel_conductor(a[:, 2], Leaf(COPPER).eta, Leaf(COPPER).k, np.float64)
    assert np.allclose(s.weight[d], f0[d], rtol=1e-12) and np.allclose(s.pdf[d], m.we[0][0], rtol=1e-12)
    # the smooth samples see the diffuse child alone: the conductor has no solid-angle density
    assert np.allclose(s.weight[~d], Leaf(DIFFUSE).refl[None], rtol=1e-12)
    assert np.allclose(s.pdf[~d], m.we[1][0] * Leaf(DIFFUSE).pdf(a[~d], s.wo[~d]), rtol=1e-12)


def test_mixture_weights_rescale_only_above_one():
    we, wp, cdf = derived_weights("mixturebsdf", weights=(0.9, 0.6))
    assert np.allclose(we, (0.6, 0.4), rtol=1e-6) and np.allclose(wp, (0.6, 0.4), rtol=1e-6) and cdf[-1] == 1
    we, wp, cdf = derived_weights("mixturebsdf", weights=(0.9, 0.6), ensure=False)
    assert we == [f32(0.9), f32(0.6)] and np.allclose(wp, (0.6, 0.4), rtol=1e-6)
    we, wp, cdf = derived_weights("mixturebsdf", weights=(0.2, 0.0, 0.3, 0.25))
    assert we == [f32(0.2), f32(0), f32(0.3), f32(0.25)] and np.allclose(wp, np.array([0.2, 0, 0.3, 0.25]) / 0.75, rtol=1e-6)


SMOOTH_CASES = {
    "blend-diffuse-gold": dict(kind="blendbsdf", children=[DIFFUSE, GOLD], weight=0.3),
    "blend-plastic-roughplastic": dict(kind="blendbsdf", children=[PLASTIC, ROUGHPLASTIC], weight=0.6),
    "mixture-3": dict(kind="mixturebsdf", children=[DIFFUSE, COPPER, GOLD], weights=(0.9, 0.6, 0.3)),
}


@pytest.mark.parametrize("name", list(SMOOTH_CASES))
def test_sampled_weight_integrates_eval_and_directions_follow_the_pdf(name):
    """E[weight 1{wo in bin}] against the integral of eval over the bin (4.5 standard errors of the estimate plus the quadrature's
    1e-3), and test_chisquare.cpp's check of the sampled directions against pdf(), as test_coatings.py runs it"""
    from scipy import stats
    m = Mix(**SMOOTH_CASES[name])
    wi = unit(WIS["oblique"]).astype(np.float64)
    n = 200000
    s = m.sample(wi, np.random.RandomState(11).rand(n, 2))
    sm = s.weight.any(1) & ~s.delta
    nb_t, nb_p, sub = 10, 20, 24
    th = (np.arange(nb_t * sub) + 0.5) / (nb_t * sub) * (np.pi / 2)
    ph = (np.arange(nb_p * sub) + 0.5) / (nb_p * sub) * 2 * np.pi
    TH, PH = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(TH) * np.cos(PH), np.sin(TH) * np.sin(PH), np.cos(TH)], -1).reshape(-1, 3)
    dw = np.sin(TH) * (np.pi / 2 / (nb_t * sub)) * (2 * np.pi / (nb_p * sub))
    w = s.wo[sm]
    it = np.clip((np.arccos(np.clip(w[:, 2], -1, 1)) / (np.pi / 2) * nb_t).astype(int), 0, nb_t - 1)
    ip = np.clip(((np.arctan2(w[:, 1], w[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nb_p).astype(int), 0, nb_p - 1)
    # E[weight 1{bin}] on a coarser grid of 2 x 4 bins
    cb = (it // 5) * 4 + ip // 5
    integral = (m.eval(wi, d).reshape(TH.shape + (3,)) * dw[..., None]).reshape(2, 5 * sub, 4, 5 * sub, 3).sum((1, 3)).reshape(8, 3)
    for b in range(8):
        x = np.zeros((n, 3)); x[np.nonzero(sm)[0][cb == b]] = s.weight[sm][cb == b]
        mean, se = x.mean(0), x.std(0) / np.sqrt(n)
        assert np.all(np.abs(mean - integral[b]) <= 4.5 * se + 1e-3 * integral[b]), (b, mean, integral[b], se)
    expect = (m.pdf(wi, d).reshape(TH.shape) * dw).reshape(nb_t, sub, nb_p, sub).sum((1, 3)) * n
    obs = np.zeros((nb_t, nb_p))
    np.add.at(obs, (it, ip), 1)
    obs, expect = obs.ravel(), expect.ravel()
    obs, expect = np.append(obs, n - sm.sum()), np.append(expect, n - expect.sum())
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


def test_the_limits():
    a, b = _pairs()
    u = np.random.RandomState(5).rand(len(a), 2)
    for c0, c1 in ((DIFFUSE, GOLD), (PLASTIC, ROUGHPLASTIC), (COPPER, DIFFUSE)):
        for w, child in ((0.0, c0), (1.0, c1)):
            m, leaf = Mix("blendbsdf", [c0, c1], weight=w), Leaf(child)
            assert np.array_equal(m.eval(a, b), leaf.eval(a, b)) and np.array_equal(m.pdf(a, b), leaf.pdf(a, b))
            s, t = m.sample(a, u), leaf.sample(a, u)
            assert np.array_equal(s.entry, np.full(len(a), int(w)))
            assert np.allclose(s.weight, t.weight, rtol=1e-12) and np.array_equal(s.pdf, t.pdf) and np.array_equal(s.wo, t.wo)
            assert np.array_equal(s.delta, t.delta)
    for child in (DIFFUSE, GOLD, PLASTIC):  # a one-child mixture of weight 1
        m, leaf = Mix("mixturebsdf", [child], weights=(1.0,)), Leaf(child)
        assert np.array_equal(m.eval(a, b), leaf.eval(a, b)) and np.array_equal(m.pdf(a, b), leaf.pdf(a, b))
        s, t = m.sample(a, u), leaf.sample(a, u)
        assert np.allclose(s.weight, t.weight, rtol=1e-12) and np.array_equal(s.pdf, t.pdf) and np.array_equal(s.wo, t.wo)


# ------------------------------------------------------------------------------------------------ 2. the cases of the GPU test
_names = list(LEAVES)
SPECS = {"blend-%s-%s" % (a, b): dict(kind="blendbsdf", children=[a, b], weight=0.3) for i, a in enumerate(_names) for b in _names[i + 1:]}
SPECS.update({
    # a delta child and a weight of zero in each; the first sums to 1.5 and is rescaled to (0.6, 0.4, 0), the second to 0.75 and is kept
    "mixture-3": dict(kind="mixturebsdf", children=["diffuse", "copper", "gold"], weights=(0.9, 0.6, 0.0)),
    "mixture-4": dict(kind="mixturebsdf", children=["plastic", "diffuse", "gold", "roughplastic"], weights=(0.2, 0.0, 0.3, 0.25)),
    "blend-bitmap-weight": dict(kind="blendbsdf", children=["diffuse", "gold"], weight_map=True),
    "blend-textured-child": dict(kind="blendbsdf", children=["diffuse", "plastic"], weight=0.3, reflectance_map=0),
    "blend-general-microfacet-child": dict(kind="blendbsdf", children=["diffuse", "aniso"], weight=0.3),
})
CASES = [(name, ts) for name in SPECS for ts in (False, True)]
N_U = 64  # sample.x lies on (k + 1/2) / 64


def case_id(c):
    return c[0] + ("-twosided" if c[1] else "")


def child_dict(name):
    return dict(ANISO_GOLD if name == "aniso" else LEAVES[name])


def blend_lattice(twosided):
    """test_coatings.lattice's 4096 items with sample.x moved onto (k + 1/2) / 64 — every weight and cdf edge of the cases is at least
    1e-3 from these (asserted below), so choosing the child costs the exclusion rule nothing — and the hit's uv: the left or the right
    texel of the two-texel bitmaps, in turns of two items"""
    wi, wo, u = lattice(twosided)
    k = np.arange(len(u))
    u = u.copy()
    u[:, 0] = ((k % N_U) + 0.5) / N_U
    uv = np.stack([np.where((k // 2) % 2 == 0, 0.25, 0.75), np.full(len(k), 0.5)], 1).astype(f32)
    return wi, wo, u.astype(f32), uv


def restatement(case, dt, half):
    name, twosided = case
    spec = SPECS[name]
    kids = []
    for i, c in enumerate(spec["children"]):
        m = child_dict(c)
        if spec.get("reflectance_map") == i:
            m["reflectance"] = tuple(TEXELS_R[half])
        kids.append(m)
    if spec["kind"] == "mixturebsdf":
        return Mix("mixturebsdf", kids, weights=spec["weights"], twosided=twosided, dt=dt)
    return Mix("blendbsdf", kids, weight=TEXELS_W[half] if spec.get("weight_map") else spec["weight"], twosided=twosided, dt=dt)


def run(case, dt):
    """eval, pdf and the sample of the restatement over the lattice, each item with the texels its uv picks"""
    wi, wo, u, uv = blend_lattice(case[1])
    spec = SPECS[case[0]]
    halves = (0, 1) if (spec.get("weight_map") or spec.get("reflectance_map") is not None) else (0,)
    parts = []
    for h in halves:
        m = restatement(case, dt, h)
        parts.append((m.eval(wi, wo), m.pdf(wi, wo), m.sample(wi, u)))
    if len(parts) == 1:
        return dict(eval=parts[0][0], pdf=parts[0][1], sample=parts[0][2])
    right = uv[:, 0] > 0.5
    (e0, p0, s0), (e1, p1, s1) = parts
    s = Sample(np.where(right[:, None], s1.wo, s0.wo), np.where(right, s1.pdf, s0.pdf), np.where(right[:, None], s1.weight, s0.weight),
               np.where(right, s1.delta, s0.delta), np.where(right, s1.margin, s0.margin))
    s.entry = np.where(right, s1.entry, s0.entry)
    return dict(eval=np.where(right[:, None], e1, e0), pdf=np.where(right, p1, p0), sample=s)


_cache = {}


def figures(case):
    """(the float64 reference with its exclusion mask `keep`, the deviations of the float32 restatement from it, the share of items
    excluded).  An item is excluded when the two precisions choose different children or leaf branches, or when it lies within MARGIN of
    a selection boundary or of a branch point inside the chosen leaf."""
    if case not in _cache:
        ref, got = run(case, np.float64), run(case, f32)
        assert got["eval"].dtype == f32 and got["sample"].wo.dtype == f32
        s, g = ref["sample"], got["sample"]
        same = (s.entry == g.entry) & (s.weight.any(1) == g.weight.any(1)) & (s.delta == g.delta)
        ref["keep"] = (s.margin >= MARGIN) & same
        _cache[case] = (ref, deviations(got, ref), float(1 - ref["keep"].mean()))
    return _cache[case]


def test_the_lattice_keeps_clear_of_every_selection_boundary():
    pts = (np.arange(N_U) + 0.5) / N_U
    for name, spec in SPECS.items():
        for h in (0, 1):
            m = restatement((name, False), np.float64, h)
            for edge in m.cdf[1:-1]:
                assert np.abs(pts - float(edge[0])).min() >= 1e-3, (name, float(edge[0]))


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_float32_restatement_against_float64(case):
    """The figures the GPU test's bounds come from, and the cap on what the exclusion rule may cost: 0.5 % of a case's items (a
    condition, not a measurement)."""
    ref, dev, excluded = figures(case)
    s = ref["sample"]
    print(case_id(case), "float32 vs float64:", dev, "excluded", excluded)
    assert MARGIN == 1e-4 and MAX_EXCLUDED == 0.005
    assert excluded <= MAX_EXCLUDED
    assert all(np.isfinite(v) for v in dev.values())
    spec = SPECS[case[0]]
    chosen = set(np.unique(s.entry[s.weight.any(1)]))
    positive = {i for i, w in enumerate(spec.get("weights", (1, 1))) if w > 0}
    assert chosen == positive  # every child of positive weight is sampled, none of weight zero
    if any(c in ("copper", "plastic") for c in spec["children"]):
        assert s.delta.any()
    wi, _, _, uv = blend_lattice(case[1])
    assert (wi[:, 2] < 0).any() == case[1] and set(np.unique(uv[:, 0])) == {f32(0.25), f32(0.75)}


# ------------------------------------------------------------------------------------------------ 5. the hosts
def test_material_dicts():
    kids = [dict(DIFFUSE), dict(COPPER)]
    m = dict(type=0, twosided=True, blend=dict(kind="blendbsdf", children=kids, weight=0.25, weight_texture=2))
    flat = expand_blends([dict(DIFFUSE), m])
    assert len(flat) == 4 and flat[1]["blend"]["children"] == [2, 3] and flat[2] == kids[0] and flat[3] == kids[1]
    assert expand_blends(flat) is flat
    b = Blend.from_dict(flat[1])
    assert (b.kind, b.n, list(b.child), b.weight[0], b.weight_texture, b.ensure_energy_conservation) == (1, 2, [2, 3, 0, 0], 0.25, 3, 0)
    assert not any(b._reserved) and Blend.from_dict(b.as_dict()).as_dict() == b.as_dict() == dict(flat[1]["blend"], children=[2, 3])
    x = Blend.from_dict(dict(kind="mixturebsdf", children=[0, 1, 2], weights=(0.5, 0.25, 0.125)))
    assert (x.kind, x.n, list(x.weight), x.ensure_energy_conservation, x.weight_texture) == (2, 3, [0.5, 0.25, 0.125, 0.0], 1, 0)
    assert Blend.from_dict(x.as_dict()).as_dict() == x.as_dict()
    assert bytes(Blend.from_dict(DIFFUSE)) == bytes(64) and Blend.from_dict(dict(kind=0, children=[])).kind == 0
    import ctypes
    assert ctypes.sizeof(Blend) == 64
    with pytest.raises(ValueError):
        Blend.from_dict(dict(kind=2, children=[0, 1, 2, 3, 4], weights=[1] * 5))
    with pytest.raises(ValueError):
        Blend.from_dict(dict(kind=2, children=[0, 1], weights=[1]))

    class D:
        materials = [dict(DIFFUSE), m]
    assert has_blends(D) and not has_blends(type("E", (), dict(materials=[dict(DIFFUSE)])))


def test_oracle_binding_refuses_blends(oracle_lib):
    from conftest import CBOX_PROPS, make_oracle
    desc = ppg_host.cbox_scene(16, 12)
    desc.materials = list(desc.materials) + [dict(type=0, blend=dict(kind="blendbsdf", children=[dict(DIFFUSE), dict(COPPER)], weight=0.5))]
    o = make_oracle(oracle_lib, **dict(CBOX_PROPS, budget=4))
    with pytest.raises(NotImplementedError):
        o.set_scene(desc)


def _blend_bytes(desc):
    return b"".join(bytes(Blend.from_dict(m)) for m in expand_blends(desc.materials))


def test_scene_file_round_trip_and_old_files(tmp_path):
    desc = ppg_host.cbox_scene(8, 8)
    n0 = len(desc.materials)
    desc.materials = list(desc.materials) + [
        dict(type=0, twosided=True, opacity=(0.5, 0.6, 0.7), blend=dict(kind="blendbsdf", children=[dict(DIFFUSE), dict(COPPER)], weight=0.25)),
        dict(type=0, blend=dict(kind="mixturebsdf", children=[0, dict(PLASTIC), n0], weights=(0.5, 0.2, 0.0), ensure_energy_conservation=False))]
    p, q = str(tmp_path / "a.ppgs"), str(tmp_path / "b.ppgs")
    ppg_host.save_scene(desc, p)
    raw = open(p, "rb").read()
    assert int(np.frombuffer(raw, np.uint32, 6, 4)[5]) & 8192 and raw.endswith(_blend_bytes(desc))
    back = ppg_host.load_scene_file(p)
    assert len(back.materials) == n0 + 5 and _blend_bytes(back) == _blend_bytes(desc)
    assert back.materials[n0]["blend"] == dict(kind="blendbsdf", children=[n0 + 2, n0 + 3], weight=0.25, weight_texture=None)
    assert back.materials[n0 + 1]["blend"]["children"] == [0, n0 + 4, n0] and "blend" not in back.materials[0]
    ppg_host.save_scene(back, q)
    assert open(q, "rb").read() == raw
    old = ppg_host.load_scene_file(os.path.join(os.path.dirname(__file__), "golden", "cbox_16x12_pinhole.ppgs"))
    assert not any("blend" in m for m in old.materials)
    ppg_host.save_scene(old, q)
    assert not int(np.frombuffer(open(q, "rb").read(), np.uint32, 6, 4)[5]) & 8192
    bad = bytearray(raw)
    bad[len(raw) - 64 * 4 + 8] = 200  # the mixture's first child index: out of range
    open(q, "wb").write(bytes(bad))
    with pytest.raises(ValueError):
        ppg_host.load_scene_file(q)


import subprocess  # noqa: E402

from test_microfacet_general import BIN, MESH, MESH_VT, REF_DATA, SPHERE, _cpp, _material_records, _save, _scene  # noqa: E402

NONE = '<string name="material" value="none"/>'
BLEND_XML = {
    "twosided-blend-diffuse-mirror": (
        '<bsdf type="twosided"> <bsdf type="blendbsdf"> <float name="weight" value="0.3"/> <bsdf type="diffuse"> <rgb name="reflectance" value="0.2, 0.5, 0.8"/> </bsdf>'
        ' <bsdf type="conductor"> %s </bsdf> </bsdf> </bsdf>' % NONE,
        dict(type=0, twosided=True), dict(kind="blendbsdf", weight=float(f32(0.3)), weight_texture=None), [0, 2]),
    "blend-defaults": ('<bsdf type="blendbsdf"> <bsdf type="diffuse"/> <bsdf type="plastic"/> </bsdf>', dict(type=0),
                       dict(kind="blendbsdf", weight=0.5, weight_texture=None), [0, 5]),
    "mask-mixture": (
        '<bsdf type="mask"> <rgb name="opacity" value="0.25"/> <bsdf type="mixturebsdf"> <string name="weights" value="0.9, 0.6;0 0.25"/>'
        ' <boolean name="ensureEnergyConservation" value="false"/> <bsdf type="diffuse"/> <bsdf type="conductor"> %s </bsdf>'
        ' <bsdf type="roughconductor"> %s <float name="alphaU" value="0.1"/> <float name="alphaV" value="0.3"/> <string name="distribution" value="ggx"/> </bsdf>'
        ' <bsdf type="plastic"> <float name="intIOR" value="1.7"/> </bsdf> </bsdf> </bsdf>' % (NONE, NONE),
        dict(type=0, opacity=(0.25, 0.25, 0.25)),
        dict(kind="mixturebsdf", weights=tuple(float(f32(v)) for v in (0.9, 0.6, 0, 0.25)), ensure_energy_conservation=False), [0, 2, 4, 5]),
}


def _load(tmp_path, body, **kw):
    desc, _, info = ppg_host.load_scene(_scene(tmp_path, body), **kw)
    return desc, info


@pytest.mark.parametrize("name", list(BLEND_XML))
def test_both_loaders_read_the_blends_and_agree(tmp_path, name):
    """the Python loader's dicts; the C++ loader (ppg_render --ppgs) writes the same ppg_material records and the same ppg_blend block
    (bit 13, the file's last); the flat file gives the dicts back; and the XML writer's output reloads to the same records"""
    bsdf, want_m, want_b, want_types = BLEND_XML[name]
    desc, info = _load(tmp_path, SPHERE % bsdf)
    assert not info["warnings"]
    i = desc.spheres[0]["material"]
    m = desc.materials[i]
    for k, v in want_m.items():
        assert m[k] == v, (k, m)
    kids = m["blend"]["children"]
    assert {k: v for k, v in m["blend"].items() if k != "children"} == want_b, m["blend"]
    assert [desc.materials[c]["type"] for c in kids] == want_types and all(c > i for c in kids)
    r, flat = _cpp(tmp_path, SPHERE % bsdf)
    assert r.returncode == 0, r.stderr
    mine = open(_save(desc, tmp_path), "rb").read()
    assert int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 8192 and int(np.frombuffer(mine, np.uint32, 6, 4)[5]) & 8192
    assert _material_records(flat) == _material_records(mine)
    blends = _blend_bytes(desc)
    assert len(blends) == 64 * len(desc.materials) and flat.endswith(blends) and mine.endswith(blends)
    if name == "mask-mixture":  # the general entry of the third child travels with it, in both
        assert int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 2048 and flat[:-len(blends)].endswith(mine[:-len(blends)][-32 * len(desc.materials):])
    back = ppg_host.load_scene_file(_save(desc, tmp_path))
    assert _blend_bytes(back) == blends
    again, _, info2 = ppg_host.load_scene(ppg_host.save_scene_xml(desc, dict(budgetType="spp", budget=8.0), str(tmp_path / "w")))
    assert not info2["warnings"]
    j = again.spheres[0]["material"]
    a, b = again.materials[j]["blend"], m["blend"]
    assert {k: v for k, v in a.items() if k != "children"} == {k: v for k, v in b.items() if k != "children"}
    rec = lambda d, c: bytes(ppg_host.bindings.Material.from_dict(d.materials[c]))  # noqa: E731
    assert [rec(again, c) for c in a["children"]] == [rec(desc, c) for c in b["children"]]
    assert rec(again, j) == rec(desc, i)


def test_nested_refs_and_a_bitmap_weight(tmp_path):
    from ppg_host import imageio
    imageio.write_pfm(str(tmp_path / "w.pfm"), np.array([[[0.2, 0.3, 0.4], [0.6, 0.7, 0.8]]], f32))
    body = ('<bsdf type="diffuse" id="paint"> <rgb name="reflectance" value="0.7, 0.1, 0.1"/> </bsdf> <bsdf type="conductor" id="metal"> %s </bsdf>'
            ' <shape type="obj"> <string name="filename" value="quad_vt.obj"/> <bsdf type="blendbsdf"> %%s <ref id="paint"/> <ref id="metal"/> </bsdf> </shape>' % NONE)
    tex = '<texture type="bitmap" name="weight"> <string name="filename" value="w.pfm"/> <float name="gamma" value="1"/> <string name="filterType" value="nearest"/> </texture>'
    desc, info = _load(tmp_path, body % tex)
    assert not info["warnings"]
    m = desc.materials[-3]
    assert m["blend"]["weight_texture"] == 0 and abs(m["blend"]["weight"] - 0.5) < 1e-6 and len(desc.textures) == 1
    assert [desc.materials[c] for c in m["blend"]["children"]] == [desc.materials[0], desc.materials[1]]
    # with a constant weight both loaders agree on the refs; the C++ loader reads no bitmaps and says so
    const = '<float name="weight" value="0.75"/>'
    desc, info = _load(tmp_path, body % const)
    r, flat = _cpp(tmp_path, body % const)
    assert r.returncode == 0, r.stderr
    mine = open(_save(desc, tmp_path), "rb").read()
    assert _material_records(flat) == _material_records(mine) and flat.endswith(_blend_bytes(desc))
    r, _ = _cpp(tmp_path, body % tex)
    assert r.returncode != 0 and "textured 'weight' is not supported" in r.stderr
    r, flat = _cpp(tmp_path, body % tex, "--lenient")
    assert r.returncode == 0 and int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 8192  # (the plug-in's default weight, 0.5)


D2 = '<bsdf type="diffuse"/> <bsdf type="diffuse"/>'
REFUSED = {  # name: (bsdf, what both loaders say)
    "blend-of-blend": ('<bsdf type="blendbsdf"> <bsdf type="blendbsdf"> %s </bsdf> <bsdf type="diffuse"/> </bsdf>' % D2, "blends of blends are not supported"),
    "mixture-of-blend": ('<bsdf type="mixturebsdf"> <string name="weights" value="1"/> <bsdf type="blendbsdf"> %s </bsdf> </bsdf>' % D2, "blends of blends are not supported"),
    "coated-child": ('<bsdf type="blendbsdf"> <bsdf type="coating"> <bsdf type="diffuse"/> </bsdf> <bsdf type="diffuse"/> </bsdf>', "coated children are not supported"),
    "coating-of-blend": ('<bsdf type="coating"> <bsdf type="blendbsdf"> %s </bsdf> </bsdf>' % D2, "coating(blendbsdf) is not supported"),
    "twosided-child": ('<bsdf type="blendbsdf"> <bsdf type="twosided"> <bsdf type="diffuse"/> </bsdf> <bsdf type="diffuse"/> </bsdf>', "blendbsdf(twosided) is not supported"),
    "mask-child": ('<bsdf type="mixturebsdf"> <string name="weights" value="1"/> <bsdf type="mask"> <bsdf type="diffuse"/> </bsdf> </bsdf>', "mixturebsdf(mask) is not supported"),
    "bumpmap-child": ('<bsdf type="blendbsdf"> <bsdf type="bumpmap"> <bsdf type="diffuse"/> </bsdf> <bsdf type="diffuse"/> </bsdf>', "blendbsdf(bumpmap) is not supported"),
    "dielectric-child": ('<bsdf type="blendbsdf"> <bsdf type="dielectric"/> <bsdf type="diffuse"/> </bsdf>', "dielectric, thindielectric and roughdielectric children are not supported"),
    "thindielectric-child": ('<bsdf type="blendbsdf"> <bsdf type="diffuse"/> <bsdf type="thindielectric"/> </bsdf>', "dielectric, thindielectric and roughdielectric children are not supported"),
    "roughdielectric-child": ('<bsdf type="mixturebsdf"> <string name="weights" value="1"/> <bsdf type="roughdielectric"/> </bsdf>', "dielectric, thindielectric and roughdielectric children are not supported"),
    "blend-one-child": ('<bsdf type="blendbsdf"> <bsdf type="diffuse"/> </bsdf>', "expected two nested BSDF instances! (found 1)"),
    "blend-three-children": ('<bsdf type="blendbsdf"> %s <bsdf type="diffuse"/> </bsdf>' % D2, "expected two nested BSDF instances! (found 3)"),
    "mixture-five-children": ('<bsdf type="mixturebsdf"> <string name="weights" value="1,1,1,1,1"/> %s %s <bsdf type="diffuse"/> </bsdf>' % (D2, D2),
                              "more than 4 nested bsdfs are not supported (found 5)"),
    "mixture-count": ('<bsdf type="mixturebsdf"> <string name="weights" value="0.5, 0.5, 0.5"/> %s </bsdf>' % D2, "BSDF count mismatch: 2 bsdfs, but specified 3 weights"),
    "mixture-no-weights": ('<bsdf type="mixturebsdf"> %s </bsdf>' % D2, "No weights were supplied!"),
    "mixture-unparsable": ('<bsdf type="mixturebsdf"> <string name="weights" value="0.5, half"/> %s </bsdf>' % D2, "Could not parse the BSDF weights!"),
    "mixture-negative": ('<bsdf type="mixturebsdf"> <string name="weights" value="0.5, -0.5"/> %s </bsdf>' % D2, "weights must be finite and not negative"),
    "mixture-not-finite": ('<bsdf type="mixturebsdf"> <string name="weights" value="0.5, inf"/> %s </bsdf>' % D2, "weights must be finite and not negative"),
    "mixture-zero-sum": ('<bsdf type="mixturebsdf"> <string name="weights" value="0, 0"/> %s </bsdf>' % D2, "The weights must sum to a value greater than zero!"),
    "blend-negative": ('<bsdf type="blendbsdf"> <float name="weight" value="-0.5"/> %s </bsdf>' % D2, "weight must be finite and not negative"),
    "blend-not-finite": ('<bsdf type="blendbsdf"> <float name="weight" value="nan"/> %s </bsdf>' % D2, "weight must be finite and not negative"),
    "procedural-weight": ('<bsdf type="blendbsdf"> <texture type="checkerboard" name="weight"/> %s </bsdf>' % D2, "'weight'"),
    "blend-unparsable": ('<bsdf type="blendbsdf"> <string name="weight" value="half"/> %s </bsdf>' % D2, "Could not parse the weight!"),
    "missing-ref": ('<bsdf type="blendbsdf"> <ref id="nowhere"/> <bsdf type="diffuse"/> </bsdf>', "no such bsdf"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_loaders_refuse_and_say_why(tmp_path, name):
    """strict loads refuse and name what they refuse; a lenient load falls back — grey diffuse for the combinator, or the nested BSDF for
    the coat around one — with a warning that says why"""
    bsdf, needle = REFUSED[name]
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, SPHERE % bsdf, data_dir=REF_DATA)
    assert needle in str(ei.value), str(ei.value)
    r, _ = _cpp(tmp_path, SPHERE % bsdf, "--data-dir", REF_DATA)
    assert r.returncode != 0 and needle in r.stderr, r.stderr
    desc, info = _load(tmp_path, SPHERE % bsdf, strict=False, data_dir=REF_DATA)
    assert any(needle in w for w in info["warnings"]), info["warnings"]
    r, flat = _cpp(tmp_path, SPHERE % bsdf, "--lenient", "--data-dir", REF_DATA)
    assert r.returncode == 0, r.stderr
    loud = subprocess.run([BIN, "--ppgs", str(tmp_path / "loud.ppgs"), "--lenient", "--data-dir", REF_DATA, _scene(tmp_path, SPHERE % bsdf)],
                          capture_output=True, text=True)  # (without -q the driver prints the loader's warnings)
    assert loud.returncode == 0 and any("warning" in line and needle in line for line in loud.stderr.splitlines()), loud.stderr


def test_a_lenient_load_keeps_a_blend_that_is_in_order(tmp_path):
    bsdf = BLEND_XML["blend-defaults"][0]
    desc, info = _load(tmp_path, SPHERE % bsdf + ' <shape type="sphere"> <bsdf type="ward"/> </shape>', strict=False)
    assert desc.materials[desc.spheres[0]["material"]]["blend"]["kind"] == "blendbsdf"
    assert not any("blendbsdf" in w for w in info["warnings"]) and any("ward" in w for w in info["warnings"])
    r, flat = _cpp(tmp_path, SPHERE % bsdf, "--lenient")
    assert r.returncode == 0 and "replaced" not in r.stderr + r.stdout and int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 8192


# what a blended material asks of the mesh it sits on: the texture coordinates, when its weight or a child reads a bitmap or a child is
# anisotropic
WEIGHT_MAP = '<texture type="bitmap" name="weight"> <string name="filename" value="w.pfm"/> <float name="gamma" value="1"/> <string name="filterType" value="nearest"/> </texture>'
ANISO_CHILD = '<bsdf type="roughconductor"> %s <float name="alphaU" value="0.1"/> <float name="alphaV" value="0.3"/> <string name="distribution" value="ggx"/> </bsdf>' % NONE
NEEDS_UVS = {
    "bitmap-weight": '<bsdf type="blendbsdf"> %s <bsdf type="diffuse"/> <bsdf type="conductor"> %s </bsdf> </bsdf>' % (WEIGHT_MAP, NONE),
    "textured-child": ('<bsdf type="blendbsdf"> <bsdf type="diffuse"> <texture type="bitmap" name="reflectance"> <string name="filename" value="w.pfm"/>'
                       ' <float name="gamma" value="1"/> </texture> </bsdf> <bsdf type="diffuse"/> </bsdf>'),
    "anisotropic-child": '<bsdf type="twosided"> <bsdf type="mixturebsdf"> <string name="weights" value="0.5, 0.5"/> <bsdf type="diffuse"/> %s </bsdf> </bsdf>' % ANISO_CHILD,
}


def _write_map(tmp_path):
    from ppg_host import imageio
    imageio.write_pfm(str(tmp_path / "w.pfm"), np.array([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]], f32))


@pytest.mark.parametrize("name", list(NEEDS_UVS))
def test_a_blend_keeps_the_texture_coordinates_of_its_mesh(tmp_path, name):
    _write_map(tmp_path)
    desc, info = _load(tmp_path, MESH_VT % NEEDS_UVS[name])
    assert not info["warnings"] and desc.texcoords is not None
    quad = np.nonzero(np.asarray(desc.tri_material) == len(desc.materials) - 3)[0]  # (the blended record stands before its two children)
    assert len(quad) == 2 and "blend" in desc.materials[-3]
    uv = np.asarray(desc.texcoords)[np.asarray(desc.indices)[quad].reshape(-1)]
    assert np.isfinite(uv).all() and {tuple(v) for v in uv.tolist()} == {(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)}
    plain, _ = _load(tmp_path, MESH_VT % '<bsdf type="blendbsdf"> <bsdf type="diffuse"/> <bsdf type="plastic"/> </bsdf>')
    assert plain.texcoords is None  # (a blend that reads nothing leaves the mesh as an untextured BSDF does)
    if name == "anisotropic-child":  # the C++ loader reads no bitmaps; the anisotropic child it reads, and keeps the mesh's uvs as well
        r, flat = _cpp(tmp_path, MESH_VT % NEEDS_UVS[name])
        assert r.returncode == 0, r.stderr
        mine = open(_save(desc, tmp_path), "rb").read()
        assert int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 16 and _material_records(flat) == _material_records(mine)
        assert flat.endswith(_blend_bytes(desc)) and mine.endswith(_blend_bytes(desc))
        (tmp_path / "cpp2.ppgs").write_bytes(flat)
        theirs = ppg_host.load_scene_file(str(tmp_path / "cpp2.ppgs"))
        assert np.array_equal(np.asarray(theirs.texcoords), np.asarray(desc.texcoords), equal_nan=True)


def test_loaders_apply_the_mesh_rules_to_blends(tmp_path):
    """the two rules of ppg_set_scene that concern the shape: an anisotropic child needs a mesh with texture coordinates, and a blend that
    reads a bitmap cannot sit on an analytic sphere, disk or cylinder"""
    _write_map(tmp_path)
    needle = "texture coordinates are required to generate tangent vectors"
    for shape in (MESH, '<shape type="rectangle"> %s </shape>'):
        with pytest.raises(mitsuba_xml.SceneError) as ei:
            _load(tmp_path, shape % NEEDS_UVS["anisotropic-child"])
        assert needle in str(ei.value)
        r, _ = _cpp(tmp_path, shape % NEEDS_UVS["anisotropic-child"])
        assert r.returncode != 0 and needle in r.stderr, r.stderr
    for shape in (SPHERE, '<shape type="disk"> %s </shape>', '<shape type="cylinder"> <float name="radius" value="1"/> %s </shape>'):
        for name in ("bitmap-weight", "textured-child"):
            with pytest.raises(mitsuba_xml.SceneError) as ei:
                _load(tmp_path, shape % NEEDS_UVS[name])
            assert "textured BSDFs are only supported on triangle meshes" in str(ei.value) and "blendbsdf" in str(ei.value)
            r, _ = _cpp(tmp_path, shape % NEEDS_UVS[name])  # (the C++ loader refuses the bitmap itself, on any shape)
            assert r.returncode != 0 and "textured" in r.stderr, r.stderr
        desc, info = _load(tmp_path, shape % NEEDS_UVS["anisotropic-child"])  # (no bitmap: an analytic shape has its own tangents)
        assert not info["warnings"]
