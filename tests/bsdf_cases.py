"""The cases of test_bsdf_layer.py and test_bsdf_layer_gpu.py: materials, and per material two deterministic item sets — LATTICE, the
lattice of test_microfacet_general_gpu.py that stays clear of every branch, and EDGE, directions and samples placed ON the branches of the
BSDF layer.  No GPU, no oracle: plain numpy and the float64 restatement (bsdf_ref.py) for the per-material thresholds.

An item is (wi, wo, u, key): wo feeds eval / pdf, u feeds sample, key = path_key(77, i, 0) with i the item's index in its material's
concatenated LATTICE + EDGE list — the key the oracle's ppgo_bsdf_sample(_ex) gives item i, from which roughdielectric draws its extra
number.  All inputs are finite, the directions unit to float32 rounding, the samples in [0, 1)."""
import functools

import numpy as np

import bsdf_ref
from test_bsdfs import GOLD, SMOOTH, roughplastic, unit
from test_microfacet_general import WIS
from test_microfacet_general_gpu import lattice, path_key

f32, f64 = np.float32, np.float64

MASKED = dict(type="diffuse", reflectance=(0.2, 0.5, 0.8), opacity=(0.9, 0.6, 0.3))
MATERIALS = list(SMOOTH) + [
    ("mirror", dict(type="mirror", reflectance=(0.9, 0.8, 0.7))),
    ("conductor-gold", dict(type="conductor", eta=GOLD["eta"], k=GOLD["k"], reflectance=(1, 1, 1))),
    ("conductor-k0", dict(type="conductor", eta=(1.5, 1.6, 1.7), k=(0, 0, 0), reflectance=(0.9, 1, 1))),
    ("dielectric-1.5", dict(type="dielectric", eta=1.5, reflectance=(0.9, 0.8, 1.0), specular=(0.7, 0.95, 0.85))),
    ("dielectric-inv1.5", dict(type="dielectric", eta=1 / 1.5, reflectance=(0.9, 0.8, 1.0), specular=(0.7, 0.95, 0.85))),
    ("dielectric-1", dict(type="dielectric", eta=1.0, reflectance=(0.9, 0.8, 1.0), specular=(0.7, 0.95, 0.85))),
    ("thindielectric-1.5", dict(type="thindielectric", eta=1.5, reflectance=(0.9, 0.8, 1.0), specular=(0.7, 0.95, 0.85))),
    ("plastic-twosided", dict(type="plastic", reflectance=(0.6, 0.3, 0.1), specular=(0.8, 0.9, 1.0), eta=1.49, twosided=True)),
    ("roughplastic-coloured-specular", roughplastic("ggx", 0.1, 1.5, reflectance=(0.6, 0.3, 0.1), specular=(0.8, 0.9, 1.0))),
    ("roughdielectric-inv1.5", dict(type="roughdielectric", alpha=0.3, eta=1 / 1.5, reflectance=(1, 1, 1), specular=(0.9, 0.95, 1.0))),
    ("roughconductor-alpha-floor", dict(GOLD, alpha=1e-4)),
    ("roughconductor-alpha-1", dict(GOLD, alpha=1.0)),
    ("mask-diffuse", MASKED),
    ("mask-0-diffuse", dict(MASKED, opacity=(0, 0, 0))),
    ("mask-1-diffuse", dict(MASKED, opacity=(1, 1, 1))),
    ("mask-twosided-roughconductor", dict(GOLD, alpha=0.6, twosided=True, opacity=(0.9, 0.6, 0.3))),
    ("mask-dielectric", dict(type="dielectric", eta=1.5, reflectance=(0.9, 0.8, 1.0), specular=(0.7, 0.95, 0.85), opacity=(0.9, 0.6, 0.3))),
]
NAMES = [n for n, _ in MATERIALS]
LEAN = ["diffuse", "twosided-diffuse", "mirror"]  # what a scene of the lean kernels may hold
COMMON_TYPES = ("diffuse", "mirror", "conductor", "roughconductor", "plastic", "roughplastic")


def in_common(mat):
    """would sort_slice put a hit on this material into the common part of a slice (csrc/ppg_kernels.h)?"""
    return mat["type"] in COMMON_TYPES and mat.get("opacity") is None


def has_eta(mat):
    return mat["type"] in ("dielectric", "thindielectric", "plastic", "roughdielectric", "roughplastic")


def _dir(z, phi):
    """the float32 direction of height z (kept to the bit, zero's sign included) and azimuth phi"""
    z = f32(z)
    s = np.sqrt(max(0.0, 1.0 - float(z) ** 2))
    return np.array([f32(s * np.cos(phi)), f32(s * np.sin(phi)), z], f32)


def edge_wi(mat):
    """-> (wi [n, 3] float32, class names [n])"""
    out = []
    for s in (1.0, -1.0):
        out.append(("normal", np.array([0, 0, s], f32)))
    for phi in (0.0, np.arctan2(0.8, 0.6)):
        out.append(("horizon+0", _dir(0.0, phi)))
        out.append(("horizon-0", _dir(-0.0, phi)))
    for z in (2.0 ** -12, 1e-4, 2.0 ** -24):
        for s in (1.0, -1.0):
            out.append(("grazing", _dir(s * z, 0.3)))
    out.append(("near-normal", np.array([2.0 ** -12, 0, np.sqrt(1 - 2.0 ** -24)], f32)))
    out.append(("near-normal", np.array([2.0 ** -24, 2.0 ** -24, 1], f32)))
    for name, w in WIS.items():
        out.append(("test_bsdfs-" + name, unit(w)))
    eta = float(f32(mat.get("eta", 1.5))) if has_eta(mat) else None
    if eta is not None and eta != 1.0:  # the side on which total internal reflection exists: inside for eta > 1, outside for eta < 1
        rel = f32(eta) if eta > 1 else f32(1) / f32(eta)
        cos_c = np.sqrt(f32(1) - f32(1) / (rel * rel), dtype=f32)
        side = -1.0 if eta > 1 else 1.0
        for k in range(-4, 5):
            out.append(("critical", _dir(f32(side) * cos_c * f32(1 + k * 2.0 ** -23), 0.7)))
        out.append(("inside-tir", _dir(side * float(cos_c) * 0.5, 0.7)))
    return np.stack([w for _, w in out]), [c for c, _ in out]


WO_CLASSES = ["reflect", "minus-wi", "refracted", "wo.z+0", "wo.z-0", "wo+z", "wo-z", "wo=wi"] + ["lattice"] * 64


def _lattice64():
    i, j = np.divmod(np.arange(64), 8)
    cz = ((j + 0.5) / 8 * 2 - 1) * 0.97
    ph = 2 * np.pi * (i + 0.37) / 8
    w = np.stack([np.sqrt(1 - cz * cz) * np.cos(ph), np.sqrt(1 - cz * cz) * np.sin(ph), cz], 1)
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(f32)


def edge_wo(mat, wi):
    """the 72 wo of one wi, float32 arithmetic where the code forms the direction itself"""
    eta = f32(mat.get("eta", 1.5)) if has_eta(mat) else f32(1.5)
    refl = np.array([-wi[0], -wi[1], wi[2]], f32)  # reflect(wi) as the plug-ins form it
    # refract(wi, cosThetaT, eta) of dielectric.cpp:304: (-s wi.x, -s wi.y, cosThetaT), in float32; at total reflection cosThetaT = 0
    _, ct, _ = bsdf_ref.fresnel_dielectric(np.array([float(wi[2])]), float(eta) if eta != 1 else 1.5)
    ct = f32(ct[0])
    e = eta if eta != 1 else f32(1.5)
    scale = -(f32(1) / e if ct < 0 else e)
    refr = np.array([scale * wi[0], scale * wi[1], ct], f32)
    nrm = np.sqrt((refr.astype(f64) ** 2).sum())
    refr = (refr / nrm).astype(f32) if nrm > 0 else -wi
    phi = np.arctan2(float(wi[1]), float(wi[0])) + 2.1
    return np.concatenate([np.stack([refl, -wi, refr, _dir(0.0, phi), _dir(-0.0, phi), np.array([0, 0, 1], f32), np.array([0, 0, -1], f32), wi]),
                           _lattice64()]).astype(f32)


U_GRID = [0.0, 2.0 ** -23, 0.25, 0.5, 0.75, 1 - 2.0 ** -23, 1 - 2.0 ** -24]  # ppg_rand returns k 2^-23; a sample divided by a probability any float < 1


def edge_u(mat, wi):
    """-> (u [m, 2] float32, class names [m]): the 7 x 7 grid, then the material's lobe thresholds at this wi and their +-1, +-2 ulp neighbours"""
    g = np.array(U_GRID, f32)
    u = [np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)]
    cls = ["u-grid"] * 49
    for axis, t in bsdf_ref.thresholds(mat, wi[None]):
        t = f32(t[0])
        if not (np.isfinite(t) and 0 < t < 1):
            continue
        nb = [t]
        for step in (1, 2):
            lo = hi = t
            for _ in range(step):
                lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(1))
            nb += [lo, hi]
        for other in (f32(0.25), f32(0.625)):
            for v in nb:
                if 0 <= v < 1:
                    u.append(np.array([[v, other] if axis == 0 else [other, v]], f32))
                    cls.append("u-threshold")
    return np.concatenate(u).astype(f32), cls


@functools.lru_cache(maxsize=None)
def edge(name):
    """-> dict(wi, wo, u [n, 3 | 2] float32, wi_class, wo_class, u_class [n]): per wi, item j takes wo j and u j of that wi's lists, the
    shorter list repeating — so eval / pdf see every wi x wo and sample sees every wi x u"""
    mat = dict(MATERIALS)[name]
    wis, wcls = edge_wi(mat)
    rows = dict(wi=[], wo=[], u=[], wi_class=[], wo_class=[], u_class=[])
    for wi, wc in zip(wis, wcls):
        wo = edge_wo(mat, wi)
        u, ucls = edge_u(mat, wi)
        m = max(len(wo), len(u))
        j = np.arange(m)
        rows["wi"].append(np.broadcast_to(wi, (m, 3)))
        rows["wo"].append(wo[j % len(wo)])
        rows["u"].append(u[j % len(u)])
        rows["wi_class"] += [wc] * m
        rows["wo_class"] += [WO_CLASSES[k % len(wo)] for k in j]
        rows["u_class"] += [ucls[k % len(u)] for k in j]
    out = {k: (np.concatenate(v).astype(f32) if k in ("wi", "wo", "u") else np.array(v)) for k, v in rows.items()}
    return out


@functools.lru_cache(maxsize=None)
def items(name):
    """LATTICE then EDGE of material `name`: dict(wi, wo, u, key, is_edge, wi_class, wo_class, u_class)"""
    lw, lo, lu = lattice()
    e = edge(name)
    n_l, n_e = len(lw), len(e["wi"])
    out = dict(wi=np.concatenate([lw, e["wi"]]), wo=np.concatenate([lo, e["wo"]]), u=np.concatenate([lu, e["u"]]))
    out["key"] = path_key(77, np.arange(n_l + n_e), 0)
    out["is_edge"] = np.arange(n_l + n_e) >= n_l
    for k in ("wi_class", "wo_class", "u_class"):
        out[k] = np.concatenate([np.array(["lattice"] * n_l), e[k]])
    for v in (out["wi"], out["wo"], out["u"]):
        assert v.dtype == f32 and np.isfinite(v).all()
    assert np.all(np.abs(np.sqrt((out["wi"].astype(f64) ** 2).sum(1)) - 1) < 4e-7) and np.all(np.abs(np.sqrt((out["wo"].astype(f64) ** 2).sum(1)) - 1) < 4e-7)
    assert np.all((out["u"] >= 0) & (out["u"] < 1)) and n_l + n_e < 20000
    return out


EDGE_CLASSES = sorted({"wi:" + c for c in ("normal", "horizon+0", "horizon-0", "grazing", "near-normal")} | {"wo:" + c for c in set(WO_CLASSES)}
                      | {"u:u-grid"})
