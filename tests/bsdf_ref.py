"""The BSDF layer in double precision, written from the formulas of the plug-ins it stands for — an independent statement that neither the
oracle nor the kernels share a header with.  Plain numpy; every function is vectorised over items and also reports the item's BRANCH
SIGNATURE: the side tests, total internal reflection yes / no, the lobe chosen, and whether the result is exactly zero.  An item whose
signature changes when a float32 input moves by one ulp sits on a branch, where a float32 and a float64 evaluation may legitimately part.

  eval_pdf(mat, wi, wo)  f |cos theta_o| and the solid-angle density of all nine plug-in types and the two adapters:
        diffuse (diffuse.cpp:110-138), mirror / conductor (conductor.cpp:220-266: delta, 0 in this measure), roughconductor
        (roughconductor.cpp:247-307), plastic (plastic.cpp:247-311), dielectric (dielectric.cpp:221-269: delta), thindielectric
        (thindielectric.cpp:166-201: delta), roughdielectric (roughdielectric.cpp:268-418), roughplastic (roughplastic.cpp:330-437),
        twosided (twosided.cpp:120-156), mask (mask.cpp:108-146)
  sample(mat, wi, u)     the delta plug-ins (conductor.cpp:268-284, dielectric.cpp:271-312, thindielectric.cpp:203-232), plastic
        (plastic.cpp:368-425), diffuse (diffuse.cpp:140-150), the diffuse branch of roughplastic (roughplastic.cpp:439-501), the mask's
        pass-through (mask.cpp:148-214) and the two-sided flip (twosided.cpp:158-180); `known` is False where the sampled microfacet
        normal would be needed (test_microfacet_general.py pins that one)
  flags(mat)             getType() & ESmooth, & (EBackSide | ETransmission), & ENull
  thresholds(mat, wi)    the sample values at which sample() changes lobe, per wi

D, G1 and the density of visible normals are test_microfacet_general.Distribution's.  A material is a Material.from_dict dictionary; its
numbers enter as the float32 values the C structure holds."""
import numpy as np

from ppg_host.bindings import Material
from test_microfacet_general import Distribution

f32, f64 = np.float32, np.float64
INV_PI = 1.0 / np.pi
DIFFUSE, TWOSIDED_DIFFUSE, MIRROR, CONDUCTOR, ROUGHCONDUCTOR, PLASTIC, DIELECTRIC, THINDIELECTRIC, ROUGHDIELECTRIC, ROUGHPLASTIC = range(10)
F_TWOSIDED, F_NONLINEAR, F_MASK, F_BECKMANN = 1, 2, 4, 8
Z_FLIP = np.array([1.0, 1.0, -1.0])


def lum(c):
    """Spectrum::getLuminance of linear sRGB (spectrum.h: 0.212671, 0.715160, 0.072169)"""
    c = np.asarray(c, f64)
    return c[..., 0] * 0.212671 + c[..., 1] * 0.715160 + c[..., 2] * 0.072169


class Params:
    def __init__(self, mat):
        m = Material.from_dict(mat)
        self.type, self.flags = int(m.type), int(m.flags)
        if self.type == TWOSIDED_DIFFUSE:
            self.type, self.flags = DIFFUSE, self.flags | F_TWOSIDED
        self.refl, self.spec, self.k, self.opacity = (np.array(list(v), f64) for v in (m.reflectance, m.specular, m.k, m.opacity))
        self.eta3 = np.array(list(m.eta), f64)
        self.eta = float(m.eta[0])
        if self.type == MIRROR:  # conductor.cpp:171-173: material "none"
            self.eta3, self.k = np.zeros(3), np.ones(3)
        self.alpha = max(float(f32(m.alpha)), float(f32(1e-4)))  # microfacet.h:135
        self.masked = bool(self.flags & F_MASK)
        transmits = self.type in (DIELECTRIC, THINDIELECTRIC, ROUGHDIELECTRIC)
        self.two_sided = bool(self.flags & F_TWOSIDED) and not transmits  # twosided.cpp:84-88: only BRDFs
        self.distr = Distribution("beckmann" if self.flags & F_BECKMANN else "ggx", self.alpha, self.alpha)
        self.slice = np.asarray(mat["slice"], f32).astype(f64) if "slice" in mat else None
        self.fdr_int = 0.0
        if self.type == PLASTIC:
            self.fdr_int = fresnel_diffuse_reflectance(1.0 / self.eta)
        if self.type == ROUGHPLASTIC:  # roughplastic.cpp:372: 1 - the slice's diffuse transmittance
            self.fdr_int = 1.0 - self.slice[-1]
        d_avg, s_avg = lum(self.refl), lum(self.spec)
        self.spec_weight = s_avg / (d_avg + s_avg) if d_avg + s_avg > 0 else 0.0  # plastic.cpp:199-200, roughplastic.cpp:275-276

    def diff_term(self):  # plastic.cpp:263-267, roughplastic.cpp:368-372
        if self.flags & F_NONLINEAR:
            return self.refl / (1.0 - self.refl * self.fdr_int)
        return self.refl / (1.0 - self.fdr_int)


# The plug-ins hold the dielectric Fresnel reflectance in a float32 and then form 1 - F (the transmitted share, plastic.cpp:263, dielectric.cpp:
# 301) and 1 - R^2 (thindielectric.cpp:163).  Towards grazing incidence F is within a few ulps of 1 and those differences keep no digit of
# a float32 evaluation, whatever the inputs: the conditioning of that ONE rounded intermediate.  F_ULPS moves every non-total reflectance by
# so many float32 ulps; the comparison (test_bsdf_layer.py) takes +-1 into its spread beside the moves of the inputs.
F_ULPS = 0


def fresnel_dielectric(cos_i, eta):
    """unpolarised Fresnel reflectance of a dielectric boundary, eta = n_inside / n_outside, cos_i > 0 from outside; -> (F, cos_t, tir)
    with cos_t signed against cos_i (util.cpp:651-681)"""
    cos_i = np.asarray(cos_i, f64)
    if eta == 1.0:
        return np.zeros_like(cos_i), -cos_i, np.zeros(cos_i.shape, bool)
    rel = np.where(cos_i > 0, eta, 1.0 / eta)  # n_transmitted / n_incident
    ct2 = 1.0 - (1.0 - cos_i * cos_i) / (rel * rel)
    tir = ct2 <= 0
    ci, ct = np.abs(cos_i), np.sqrt(np.maximum(ct2, 0.0))
    with np.errstate(all="ignore"):
        rs = (ci - rel * ct) / (ci + rel * ct)
        rp = (rel * ci - ct) / (rel * ci + ct)
    F = np.where(tir, 1.0, 0.5 * (rs * rs + rp * rp))
    if F_ULPS:  # (see F_ULPS)
        F = np.where(tir, F, np.clip(F + F_ULPS * np.spacing(F.astype(f32)).astype(f64), 0.0, 1.0))
    return F, np.where(tir, 0.0, np.where(cos_i > 0, -ct, ct)), tir


def fresnel_diffuse_reflectance(eta, n=1 << 18):
    """2 int_0^1 F(mu, eta) mu dmu (util.cpp:683-737 without the fast fit), Simpson's rule in mu on each side of the critical angle"""
    def simpson(a, b):
        if not b > a:
            return 0.0
        mu = np.linspace(a, b, n + 1)
        w = np.ones(n + 1)
        w[1:-1:2], w[2:-1:2] = 4, 2
        return float((w * fresnel_dielectric(mu, eta)[0] * mu).sum() * (b - a) / n / 3) * 2
    crit = np.sqrt(max(0.0, 1.0 - eta * eta)) if eta < 1 else 0.0
    return crit * crit + simpson(crit, 1.0)  # (F = 1 below the critical angle)


def fresnel_conductor(cos_i, eta, k):
    """exact unpolarised reflectance of a conductor (util.cpp:739-761), per channel: [n] x [3] -> [n, 3]"""
    c = np.asarray(cos_i, f64)[:, None]
    c2 = c * c
    s2 = 1.0 - c2
    t1 = eta * eta - k * k - s2
    a2pb2 = np.sqrt(np.maximum(t1 * t1 + 4.0 * k * k * eta * eta, 0.0))
    a = np.sqrt(np.maximum(0.5 * (a2pb2 + t1), 0.0))
    with np.errstate(all="ignore"):
        term1, term2 = a2pb2 + c2, 2.0 * a * c
        rs2 = (term1 - term2) / (term1 + term2)
        term3, term4 = a2pb2 * c2 + s2 * s2, term2 * s2
        rp2 = rs2 * (term3 - term4) / (term3 + term4)
    return 0.5 * (rp2 + rs2)


def cubic_interp(x, values):
    """Catmull-Rom spline through `values` on [0, 1], one-sided differences at the ends, 0 outside (spline.cpp:23-60)"""
    x = np.asarray(x, f64)
    size = len(values)
    t = x * (size - 1)
    k = np.clip(np.nan_to_num(t).astype(np.int64), 0, size - 2)
    f0, f1 = values[k], values[k + 1]
    d0 = np.where(k > 0, 0.5 * (values[k + 1] - values[np.maximum(k - 1, 0)]), f1 - f0)
    d1 = np.where(k + 2 < size, 0.5 * (values[np.minimum(k + 2, size - 1)] - values[k]), f1 - f0)
    t = t - k
    t2, t3 = t * t, t * t * t
    r = (2 * t3 - 3 * t2 + 1) * f0 + (-2 * t3 + 3 * t2) * f1 + (t3 - 2 * t2 + t) * d0 + (t3 - t2) * d1
    return np.where((x >= 0) & (x <= 1), r, 0.0)


def rough_transmittance(P, cos_t):
    """RoughTransmittance::eval for the material's alpha and eta: its slice over cos^(1/4) (rtrans.h:185-196, 233)"""
    cos_t = np.asarray(cos_t, f64)
    r = np.clip(cubic_interp(np.abs(cos_t) ** 0.25, P.slice[:-1]), 0.0, 1.0)  # (the slice's last entry is its diffuse transmittance)
    return np.where(cos_t >= 0, r, 0.0)


def plastic_ps(P, cos_i):
    Fi = fresnel_dielectric(cos_i, P.eta)[0]
    w = P.spec_weight
    with np.errstate(all="ignore"):
        return Fi * w / (Fi * w + (1 - Fi) * (1 - w)), Fi  # plastic.cpp:298-300


def roughplastic_ps(P, cos_i):
    ps = 1.0 - rough_transmittance(P, cos_i)
    w = P.spec_weight
    with np.errstate(all="ignore"):
        return ps * w / (ps * w + (1 - ps) * (1 - w))  # roughplastic.cpp:406-412


def thin_R(P, cos_i):
    R = fresnel_dielectric(np.abs(cos_i), P.eta)[0]
    with np.errstate(all="ignore"):
        return np.where(R < 1, R + (1 - R) ** 2 * R / (1 - R * R), R)  # thindielectric.cpp:160-164: R + TRT + TR^3T + ..


def _norm(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v * v).sum(1))[:, None]


def _dot(a, b):
    return (a * b).sum(1)


def _signum(v):
    """math::signum: the sign bit, never zero"""
    return np.where(np.signbit(v), -1.0, 1.0)


class _Sig:
    def __init__(self, n):
        self.v, self.bit = np.zeros(n, np.int64), 0

    def mark(self, cond):
        self.v |= np.asarray(cond, bool).astype(np.int64) << self.bit
        self.bit += 1


def _eval_pdf_one(P, wi, wo, S):
    n = len(wi)
    wiz, woz = wi[:, 2], wo[:, 2]
    zero3, zero = np.zeros((n, 3)), np.zeros(n)
    D = P.distr
    with np.errstate(all="ignore"):
        if P.type == DIFFUSE:
            ok = (wiz > 0) & (woz > 0)
            S.mark(wiz > 0); S.mark(woz > 0)
            p = np.where(ok, INV_PI * woz, 0.0)
            return p[:, None] * P.refl, p
        if P.type in (MIRROR, CONDUCTOR, DIELECTRIC, THINDIELECTRIC):
            return zero3, zero
        if P.type == PLASTIC:
            ok = (wiz > 0) & (woz > 0)
            S.mark(wiz > 0); S.mark(woz > 0)
            ps, Fi = plastic_ps(P, wiz)
            Fo = fresnel_dielectric(woz, P.eta)[0]
            v = INV_PI * woz / (P.eta * P.eta) * (1 - Fi) * (1 - Fo)
            return np.where(ok, v, 0.0)[:, None] * P.diff_term(), np.where(ok, INV_PI * woz * (1 - ps), 0.0)
        if P.type == ROUGHCONDUCTOR:
            ok = (wiz > 0) & (woz > 0)
            S.mark(wiz > 0); S.mark(woz > 0)
            H = _norm(wi + wo)
            Dm, Gi, Go = D.D(H), D.G1(wi, H), D.G1(wo, H)
            F = fresnel_conductor(_dot(wi, H), P.eta3, P.k) * P.refl
            f = np.where(ok & (Dm != 0), Dm * Gi * Go / (4 * wiz), 0.0)
            return np.nan_to_num(F) * f[:, None], np.where(ok, Dm * Gi / (4 * wiz), 0.0)
        if P.type == ROUGHPLASTIC:
            ok = (wiz > 0) & (woz > 0)
            S.mark(wiz > 0); S.mark(woz > 0)
            H = _norm(wi + wo)
            Dm, Gi, Go = D.D(H), D.G1(wi, H), D.G1(wo, H)
            F, _, tir = fresnel_dielectric(_dot(wi, H), P.eta)
            spec = F * Dm * Gi * Go / (4 * wiz)
            T12, T21 = rough_transmittance(P, wiz), rough_transmittance(P, woz)
            diff = INV_PI * woz * T12 * T21 / (P.eta * P.eta)
            f = np.where(ok, spec, 0.0)[:, None] * P.spec + np.where(ok, diff, 0.0)[:, None] * P.diff_term()
            ps = roughplastic_ps(P, wiz)
            p = D.pdf_visible(wi, H) / (4 * _dot(wo, H)) * ps + (1 - ps) * INV_PI * woz
            return f, np.where(ok, p, 0.0)
        if P.type == ROUGHDIELECTRIC:
            reflect = wiz * woz > 0
            rel = np.where(wiz > 0, P.eta, 1.0 / P.eta)
            H0 = _norm(np.where(reflect[:, None], wi + wo, wi + wo * rel[:, None]))
            H = H0 * _signum(H0[:, 2])[:, None]
            S.mark(wiz > 0); S.mark(wiz == 0); S.mark(reflect); S.mark(np.signbit(H0[:, 2]))
            Dm, Gi, Go = D.D(H), D.G1(wi, H), D.G1(wo, H)
            F, _, tir = fresnel_dielectric(_dot(wi, H), P.eta)
            S.mark(tir)
            fr = F * Dm * Gi * Go / (4 * np.abs(wiz))
            sd = _dot(wi, H) + rel * _dot(wo, H)
            ft = np.abs((1 - F) * Dm * Gi * Go * rel * rel * _dot(wi, H) * _dot(wo, H) / (wiz * sd * sd)) / (rel * rel)
            live = (wiz != 0) & (Dm != 0)
            f = np.where((live & reflect)[:, None], fr[:, None] * P.refl, np.where((live & ~reflect)[:, None], ft[:, None] * P.spec, 0.0))
            dwh = np.where(reflect, 1 / (4 * _dot(wo, H)), rel * rel * _dot(wo, H) / (sd * sd))
            prob = D.pdf_visible(wi * _signum(wiz)[:, None], H) * np.where(reflect, F, 1 - F)
            return f, np.abs(prob * dwh)
    raise ValueError(P.type)


def eval_pdf(mat, wi, wo):
    """-> (f |cos theta_o| [n, 3], pdf [n], signature [n])"""
    P = mat if isinstance(mat, Params) else Params(mat)
    wi, wo = np.array(wi, f64).reshape(-1, 3), np.array(wo, f64).reshape(-1, 3)
    S = _Sig(len(wi))
    if P.two_sided:  # twosided.cpp:120-156: the nested BRDF from the other side unless wi is above
        flip = ~(wi[:, 2] > 0)
        S.mark(flip)
        wi, wo = np.where(flip[:, None], wi * Z_FLIP, wi), np.where(flip[:, None], wo * Z_FLIP, wo)
    f, p = _eval_pdf_one(P, wi, wo, S)
    if P.masked:  # mask.cpp:108-146
        f, p = f * P.opacity, p * lum(P.opacity)
    S.mark(f.any(1)); S.mark(p != 0)
    return f, p, S.v


def cosine_hemisphere(u):
    """Shirley and Chiu's concentric map of the square to the disk, lifted to the hemisphere (warp.cpp:43-51, 77-107); z = 0 becomes
    1e-10f (warp.cpp:48-49)"""
    r1, r2 = 2 * u[:, 0] - 1, 2 * u[:, 1] - 1
    with np.errstate(all="ignore"):
        first = r1 * r1 > r2 * r2
        r = np.where(first, r1, r2)
        phi = np.where(first, (np.pi / 4) * (r2 / r1), np.pi / 2 - (r1 / r2) * (np.pi / 4))
    phi = np.where((r1 == 0) & (r2 == 0), 0.0, phi)
    r = np.where((r1 == 0) & (r2 == 0), 0.0, r)
    px, py = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(np.maximum(0.0, 1 - px * px - py * py))
    return np.stack([px, py, np.where(z == 0, f64(f32(1e-10)), z)], 1), first


def _sample_one(P, wi, u, S):
    n = len(wi)
    wiz = wi[:, 2]
    out = dict(wo=np.zeros((n, 3)), weight=np.zeros((n, 3)), pdf=np.zeros(n), eta=np.ones(n), delta=np.zeros(n, bool), null=np.zeros(n, bool),
               known=np.ones(n, bool))
    refl_dir = wi * np.array([-1.0, -1.0, 1.0])
    with np.errstate(all="ignore"):
        if P.type == DIFFUSE:
            ok = wiz > 0
            S.mark(ok)
            wo, first = cosine_hemisphere(u)
            S.mark(first & ok)
            out.update(wo=np.where(ok[:, None], wo, 0.0), pdf=np.where(ok, INV_PI * wo[:, 2], 0.0), weight=np.where(ok[:, None], P.refl, 0.0))
        elif P.type in (MIRROR, CONDUCTOR):
            ok = wiz > 0
            S.mark(ok)
            F = fresnel_conductor(wiz, P.eta3, P.k) * P.refl
            out.update(wo=np.where(ok[:, None], refl_dir, 0.0), pdf=ok.astype(f64), delta=ok, weight=np.where(ok[:, None], np.nan_to_num(F), 0.0))
        elif P.type == PLASTIC:
            ok = wiz > 0
            ps, Fi = plastic_ps(P, wiz)
            spec = u[:, 0] < ps
            S.mark(ok); S.mark(spec & ok)
            ud = np.stack([(u[:, 0] - ps) / (1 - ps), u[:, 1]], 1)
            wd, first = cosine_hemisphere(ud)
            S.mark(first & ok & ~spec)
            Fo = fresnel_dielectric(wd[:, 2], P.eta)[0]
            wdiff = (1 - Fi) * (1 - Fo) / (P.eta * P.eta) / (1 - ps)
            w = np.where(spec[:, None], (Fi / ps)[:, None] * P.spec, wdiff[:, None] * P.diff_term())
            out.update(wo=np.where(ok[:, None], np.where(spec[:, None], refl_dir, wd), 0.0), delta=ok & spec,
                       pdf=np.where(ok, np.where(spec, ps, (1 - ps) * INV_PI * wd[:, 2]), 0.0), weight=np.where(ok[:, None], w, 0.0))
        elif P.type == DIELECTRIC:
            F, ct, tir = fresnel_dielectric(wiz, P.eta)
            refl = u[:, 0] <= F
            S.mark(refl); S.mark(tir); S.mark(ct < 0)
            inward = ct < 0  # the refracted ray enters the inside
            scale = -np.where(inward, 1 / P.eta, P.eta)
            wt = np.stack([scale * wi[:, 0], scale * wi[:, 1], ct], 1)
            factor = np.where(inward, 1 / P.eta, P.eta)  # radiance scales with the squared index ratio (dielectric.cpp:303-307)
            out.update(wo=np.where(refl[:, None], refl_dir, wt), pdf=np.where(refl, F, 1 - F), delta=np.ones(n, bool),
                       eta=np.where(refl, 1.0, np.where(inward, P.eta, 1 / P.eta)),
                       weight=np.where(refl[:, None], P.refl, (factor * factor)[:, None] * P.spec))
        elif P.type == THINDIELECTRIC:
            R = thin_R(P, wiz)
            refl = u[:, 0] <= R
            S.mark(refl)
            out.update(wo=np.where(refl[:, None], refl_dir, -wi), pdf=np.where(refl, R, 1 - R), delta=np.ones(n, bool), null=~refl,
                       weight=np.where(refl[:, None], P.refl, P.spec))
        elif P.type == ROUGHPLASTIC:
            ok = wiz > 0
            ps = roughplastic_ps(P, wiz)
            spec = u[:, 1] < ps
            S.mark(ok); S.mark(spec & ok)
            ud = np.stack([u[:, 0], (u[:, 1] - ps) / (1 - ps)], 1)
            wd, first = cosine_hemisphere(ud)
            S.mark(first & ok & ~spec)
            S2 = _Sig(n)
            f, p = _eval_pdf_one(P, wi, wd, S2)
            good = ok & ~spec & (p != 0)
            S.mark(good)
            out.update(wo=np.where((ok & ~spec)[:, None], wd, 0.0), pdf=np.where(good, p, 0.0), weight=np.where(good[:, None], f / p[:, None], 0.0),
                       known=~(ok & spec))
        else:  # roughconductor, roughdielectric: the sampled normal is test_microfacet_general.py's subject
            out["known"] = np.zeros(n, bool)
            S.mark(wiz > 0); S.mark(wiz == 0)
    return out


def sample(mat, wi, u):
    """-> dict(wo [n, 3], weight [n, 3], pdf, eta, delta, null, known, sig)"""
    P = mat if isinstance(mat, Params) else Params(mat)
    wi, u = np.array(wi, f64).reshape(-1, 3), np.array(u, f64).reshape(-1, 2)
    n = len(wi)
    S = _Sig(n)
    prob = lum(P.opacity) if P.masked else 1.0
    through = np.zeros(n, bool)
    if P.masked:  # mask.cpp:148-214: the sample picks the nested BSDF with probability `prob`, and reuses what is left of it
        through = ~(u[:, 0] < prob)
        S.mark(through)
        with np.errstate(all="ignore"):
            u = np.stack([u[:, 0] / prob, u[:, 1]], 1)
        u = np.where(through[:, None], 0.5, u)
    flipped = np.zeros(n, bool)
    wn = wi
    if P.two_sided:  # twosided.cpp:158-180
        flipped = wi[:, 2] < 0
        S.mark(flipped)
        wn = np.where(flipped[:, None], wi * Z_FLIP, wi)
    o = _sample_one(P, wn, u, S)
    unflip = flipped & o["weight"].any(1) & (o["pdf"] != 0)
    o["wo"] = np.where(unflip[:, None], o["wo"] * Z_FLIP, o["wo"])
    if P.masked:
        with np.errstate(all="ignore"):
            o["weight"] = np.where(through[:, None], (1 - P.opacity) / (1 - prob), o["weight"] * P.opacity / prob)
        o["pdf"] = np.where(through, 1 - prob, o["pdf"] * prob)
        o["wo"] = np.where(through[:, None], -wi, o["wo"])
        o["eta"] = np.where(through, 1.0, o["eta"])
        o["delta"] = o["delta"] | through
        o["null"] = np.where(through, True, o["null"])
        o["known"] = o["known"] | through
    S.mark(o["weight"].any(1)); S.mark(o["pdf"] != 0)
    o["sig"] = S.v
    return o


def flags(mat):
    """-> (smooth, backside or transmission, has a null component): bsdf.h's getType() & ESmooth, & (EBackSide | ETransmission), & ENull"""
    P = mat if isinstance(mat, Params) else Params(mat)
    smooth = P.type in (DIFFUSE, ROUGHCONDUCTOR, PLASTIC, ROUGHDIELECTRIC, ROUGHPLASTIC)
    back = bool(P.flags & (F_TWOSIDED | F_MASK)) or P.type in (DIELECTRIC, THINDIELECTRIC, ROUGHDIELECTRIC)
    return smooth, back, P.masked or P.type == THINDIELECTRIC


def thresholds(mat, wi):
    """the sample values at which sample() changes lobe for each wi: a list of (axis, float64 [n]); NaN where there is none"""
    P = mat if isinstance(mat, Params) else Params(mat)
    wi = np.array(wi, f64).reshape(-1, 3)
    z = wi[:, 2]
    if P.two_sided:
        z = np.where(z < 0, -z, z)
    prob = lum(P.opacity) if P.masked else 1.0
    out = []
    if P.masked:
        out.append((0, np.full(len(z), prob)))
    with np.errstate(all="ignore"):
        if P.type == PLASTIC:
            out.append((0, np.where(z > 0, plastic_ps(P, z)[0] * prob, np.nan)))
        if P.type == ROUGHPLASTIC:
            out.append((1, np.where(z > 0, roughplastic_ps(P, z), np.nan)))
        if P.type == DIELECTRIC:
            out.append((0, fresnel_dielectric(z, P.eta)[0] * prob))
        if P.type == THINDIELECTRIC:
            out.append((0, thin_R(P, z) * prob))
    return out
