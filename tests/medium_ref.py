"""What tests/test_media.py (CPU) and tests/test_media_gpu.py share: a numpy restatement, generic in dtype, of the reference's homogeneous
medium and its two phase functions, written from the reference's text; the media and the items of the item-by-item test; the margins.
Not a test module.

Restated (mitsuba/src/medium/homogeneous.cpp, mitsuba/src/librender/medium.cpp, mitsuba/src/phase/isotropic.cpp, hg.cpp):
  derive(medium)            sigmaT = sigmaA + sigmaS; the default mediumSamplingWeight (homogeneous.cpp:168-184); `single`'s density (:188-204)
  sample_distance(...)      HomogeneousMedium::sampleDistance (:275-352) on a ray that starts at the origin, mint = 0, maxt = length
  eval_transmittance(...)   HomogeneousMedium::evalTransmittance (:266-273)
  phase_eval / phase_sample IsotropicPhaseFunction, HGPhaseFunction (hg.cpp:74-110, the |g| < Epsilon branch included)
Evaluated in float32 it follows the device code's order of operations with numpy's exp / log in place of the project's deterministic ones;
in float64 it is the reference that is not the project's float code.

Margins.  The device is compared against float64 within 8 x the largest difference between the float32 and the float64 evaluation over
the SAME items (figures(), measured on the CPU, never from the kernel), per quantity and per item class: "edge" — the first 64 items of a
medium, whose random numbers sit on the edges — and "random".  A quantity that spans decades (t, pdf_success, the phase value and density)
is compared relative to max(|float64 value|, RELATIVE[quantity]); the others, which live in [0, 1] or [-1, 1], absolutely.  The figures
are those of ill-conditioned steps, not of sloppy arithmetic: 1 - u / weight cancels where u nears the weight (t), sqrt(1 - cos^2) where
hg's cosine nears 1 (wo, g = 0.95), (1 - g)^2 where its forward peak is evaluated (phase).  Measured here (python tests/medium_ref.py):
  edge    t 4.3e-06  pdf_success 3.0e-05  pdf_failure 8.7e-08  transmittance 3.9e-07  eval_transmittance 8.6e-08  wo 9.1e-04  phase 8.5e-05
  random  t 2.3e-04  pdf_success 1.8e-05  pdf_failure 1.4e-07  transmittance 6.2e-07  eval_transmittance 1.1e-07  wo 2.7e-05  phase 1.2e-04
and at most 0.61 % of a medium's items are unsure.
Items float64 cannot decide are left out ("unsure"): the sampled distance within the margin of the ray's length, or the first random number
within it of the sampling weight (the branch between "a distance is sampled" and "none is"); items whose float64 value is not finite (a
channel without extinction over an infinite segment gives 0 * inf = NaN in the reference) are compared by their not being finite.  The item
set keeps the unsure share far below the 1 % the test allows (unsure_share(), asserted in tests/test_media.py).
"""
import numpy as np

EPSILON = 1e-4  # constants.h
INV_FOURPI = 0.07957747154594766788
BALANCE, SINGLE, MANUAL = 0, 1, 2
ISOTROPIC, HG = 0, 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def derive(medium, dtype=np.float64):
    """(sigmaS, sigmaT, sampling weight, sampling density, strategy, phase, g) of a medium dict (ppg_host.bindings.Medium's keys), the
    coefficients rounded to float32 first — what ppg_medium carries — and everything else in `dtype`."""
    from ppg_host.bindings import Medium
    m = Medium.from_dict(medium)
    f = dtype
    # (configuration, not sampling: the constructor's arithmetic is single precision in the reference and in the library alike, and both
    # evaluations below start from the same float32 table)
    f32 = np.float32
    sa, ss = np.array(list(m.sigma_a), f32), np.array(list(m.sigma_s), f32)
    st = sa + ss
    weight = f32(m.sampling_weight)
    if weight == -1:
        with np.errstate(all="ignore"):
            for c in range(3):
                if st[c] != 0 and ss[c] / st[c] > weight:
                    weight = ss[c] / st[c]
        if weight > 0:
            weight = max(weight, f32(0.5))
        if weight < 0:  # (no extinction at all: the reference keeps -1 and never samples a distance; the library says 0)
            weight = f32(0)
    density = f32(0)
    if m.strategy == SINGLE:
        channel = int(np.argmin(st)) if m.channel < 0 else m.channel  # (argmin: the first of equal ones, as the reference's loop)
        density = st[channel]
    elif m.strategy == MANUAL:
        density = f32(m.sampling_density)
    return dict(sigma_s=ss.astype(f), sigma_t=st.astype(f), weight=f(weight), density=f(density), strategy=int(m.strategy), phase=int(m.phase), g=f(f32(m.g)))


def _exp(x):
    with np.errstate(all="ignore"):
        return np.exp(x)


def eval_transmittance(D, length):
    """[n, 3]: exp(-sigmaT * length) per channel, 1 where sigmaT = 0"""
    f = D["sigma_t"].dtype.type
    length = np.asarray(length, f)[:, None]
    with np.errstate(all="ignore"):
        tr = _exp(D["sigma_t"][None, :] * -length)
    return np.where(D["sigma_t"][None, :] != 0, tr, f(1))


def sample_distance(D, length, u0, u1, direction):
    """sampleDistance per item: dict(success, t, pdf_success, pdf_failure, transmittance [n, 3], sampled (the distance before it is cut at the
    ray's length)).  u1 is read only by `balance`, only where u0 lies below the sampling weight.  direction [n, 3]: the ray's (the "no
    forward progress" rule compares the event's position with the origin)."""
    f = D["sigma_t"].dtype.type
    length, u0, u1 = np.asarray(length, f), np.asarray(u0, f), np.asarray(u1, f)
    st, w = D["sigma_t"], D["weight"]
    inside = u0 < w
    with np.errstate(all="ignore"):
        rand = u0 / w
        density = np.full(u0.shape, D["density"], f)
        if D["strategy"] == BALANCE:
            channel = np.minimum((u1 * f(3)).astype(np.int32), 2)
            density = st[channel]
        sampled = np.where(inside, -np.log(f(1) - rand) / density, f(np.inf)).astype(f)
        success = sampled < length
        dist = np.where(success, sampled, length).astype(f)
        p = np.asarray(direction, f) * dist[:, None]
        success &= ~np.all(p == 0, axis=1)
        if D["strategy"] == BALANCE:
            pf, ps = np.zeros_like(dist), np.zeros_like(dist)
            for c in range(3):
                tmp = _exp(-st[c] * dist)
                pf = pf + tmp
                ps = ps + st[c] * tmp
            pf, ps = pf / f(3), ps / f(3)
        else:
            pf = _exp(-density * dist)
            ps = density * pf
        tr = _exp(st[None, :] * -dist[:, None])
        ps = ps * w
        pf = w * pf + (f(1) - w)
        # Spectrum::max() = std::max over the channels in order: a NaN channel loses every comparison it is the right-hand side of
        mx = tr[:, 0]
        for c in (1, 2):
            mx = np.where(mx < tr[:, c], tr[:, c], mx)
        tr = np.where((mx < f(1e-20))[:, None], f(0), tr)
    return dict(success=success, t=dist, pdf_success=ps.astype(f), pdf_failure=pf.astype(f), transmittance=tr.astype(f), sampled=sampled)


def phase_eval(D, wi, wo):
    f = D["sigma_t"].dtype.type
    wi, wo = np.asarray(wi, f), np.asarray(wo, f)
    if D["phase"] == ISOTROPIC:
        return np.full(wi.shape[0], f(INV_FOURPI), f)
    g = D["g"]
    temp = f(1) + g * g + f(2) * g * np.sum(wi * wo, axis=1)
    return (f(INV_FOURPI) * (f(1) - g * g) / (temp * np.sqrt(temp))).astype(f)


def phase_sample(D, wi, sx, sy):
    """(wo [n, 3], pdf [n]) of the 2-D sample (sx, sy); the sampled value is 1"""
    f = D["sigma_t"].dtype.type
    wi, sx, sy = np.asarray(wi, f), np.asarray(sx, f), np.asarray(sy, f)
    pi = f(np.float32(np.pi))  # M_PI of a single-precision build
    if D["phase"] == ISOTROPIC:
        z = f(1) - f(2) * sy
        r = np.sqrt(np.maximum(f(0), f(1) - z * z))
        phi = f(2) * pi * sx
        wo = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(f)
        return wo, np.full(wi.shape[0], f(INV_FOURPI), f)
    g = D["g"]
    if abs(g) < f(EPSILON):
        cos_t = f(1) - f(2) * sx
    else:
        sqr = (f(1) - g * g) / (f(1) - g + f(2) * g * sx)
        cos_t = (f(1) + g * g - sqr * sqr) / (f(2) * g)
    sin_t = np.sqrt(np.maximum(f(0), f(1) - cos_t * cos_t))
    phi = f(2) * pi * sy
    a = -wi  # Frame(-wi): coordinateSystem, util.cpp:592-601
    first = np.abs(a[:, 0]) > np.abs(a[:, 1])
    with np.errstate(all="ignore"):
        inv1 = f(1) / np.sqrt(a[:, 0] * a[:, 0] + a[:, 2] * a[:, 2])
        inv2 = f(1) / np.sqrt(a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
    zero = np.zeros_like(inv1)
    with np.errstate(all="ignore"):
        c = np.where(first[:, None], np.stack([a[:, 2] * inv1, zero, -a[:, 0] * inv1], 1), np.stack([zero, a[:, 2] * inv2, -a[:, 1] * inv2], 1))
    b = np.cross(c, a)
    wo = (b * (sin_t * np.cos(phi))[:, None] + c * (sin_t * np.sin(phi))[:, None] + a * np.asarray(cos_t, f)[:, None]).astype(f)
    return wo, phase_eval(D, wi, wo)


def evaluate(medium, items, dtype):
    """Everything ppg_debug_medium returns, for one medium dict and its items (ITEM fields length, wi, u), in `dtype`"""
    D = derive(medium, dtype)
    wi = np.asarray(items["wi"], dtype)
    u = np.asarray(items["u"], dtype)
    out = sample_distance(D, np.asarray(items["length"], dtype), u[:, 0], u[:, 1], -wi)
    out["eval_transmittance"] = eval_transmittance(D, np.asarray(items["length"], dtype))
    out["wo"], out["phase_pdf"] = phase_sample(D, wi, u[:, 2], u[:, 3])
    out["phase_eval"] = phase_eval(D, wi, out["wo"])
    out["weight"] = D["weight"]
    return out


# ---------------------------------------------------------------------------------------------------------------- media and items
def _phase(g):
    return dict(phase="isotropic") if g is None else dict(phase="hg", g=g)


MEDIA = [  # (name, medium dict): grey and coloured, a channel without extinction, a pure absorber, albedo 1, each strategy, every g
    ("grey balance", dict(sigma_a=0.5, sigma_s=1.5, **_phase(None))),
    ("coloured balance hg -0.9", dict(sigma_a=(0.2, 0.5, 1.0), sigma_s=(1.0, 2.0, 0.5), **_phase(-0.9))),
    ("zero channel balance hg 0", dict(sigma_a=(0.5, 0.0, 0.25), sigma_s=(1.0, 0.0, 2.0), **_phase(0.0))),
    ("pure absorber", dict(sigma_a=(1.0, 2.0, 3.0), sigma_s=0.0, **_phase(1e-5))),
    ("albedo one hg 0.3", dict(sigma_t=(2.0, 3.0, 4.0), albedo=1.0, scale=0.5, **_phase(0.3))),
    ("single hg 0.95", dict(sigma_a=(0.3, 0.2, 0.1), sigma_s=(3.0, 2.0, 1.0), strategy="single", **_phase(0.95))),
    ("single channel 0", dict(sigma_a=(0.3, 0.2, 0.1), sigma_s=(3.0, 2.0, 1.0), strategy="single", channel=0, **_phase(None))),
    ("manual", dict(sigma_a=0.25, sigma_s=(0.5, 1.0, 1.5), strategy="manual", sampling_density=1.25, sampling_weight=0.7, **_phase(1e-5))),
    ("zero channel single", dict(sigma_a=(0.0, 0.5, 0.5), sigma_s=(0.0, 1.0, 2.0), strategy="single", channel=1, **_phase(0.3))),
]
N_ITEMS = 4096
ITEM_DTYPE = np.dtype([("medium", "<i4"), ("length", "<f4"), ("wi", "<f4", 3), ("u", "<f4", 4)])  # = ppg_host.bindings.DEBUG_MEDIUM_ITEM_DTYPE
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)


def items_for(index, medium):
    """N_ITEMS items of medium `index`: lengths tiny, about 1 / sigma, 1e4 / sigma and infinite; random numbers 0, just below 1, on both
    sides of the sampling weight, and random; random unit wi, the coordinate axes among them"""
    rng = np.random.default_rng(1000 + index)
    D = derive(medium, np.float64)
    sigma = float(max(D["sigma_t"].max(), 1e-3))
    it = np.zeros(N_ITEMS, ITEM_DTYPE)
    it["medium"] = index
    lengths = np.array([1e-6 / sigma, 1.0 / sigma, 1e4 / sigma, np.inf], np.float32)
    it["length"] = lengths[np.arange(N_ITEMS) % 4]
    it["length"][N_ITEMS // 2:] *= rng.uniform(0.25, 4.0, N_ITEMS - N_ITEMS // 2).astype(np.float32)
    wi = rng.normal(size=(N_ITEMS, 3))
    wi[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    it["wi"] = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    u = rng.uniform(0.0, 1.0, (N_ITEMS, 4)).astype(np.float32)
    w = np.float32(D["weight"])
    special = np.array([0.0, BELOW_ONE, np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(2)), w * np.float32(0.999), w * np.float32(1.001)], np.float32)
    special = np.where(special > 1, np.float32(0.5), special)  # (a weight of 1 has nothing above it)
    for k in range(4):  # the first 64 items of each column walk the special values, out of step with each other and with the lengths
        u[:64, k] = special[(np.arange(64) // (k + 1) + k) % len(special)] if k == 0 else np.array([0.0, BELOW_ONE, 0.5, 0.25, 0.75], np.float32)[(np.arange(64) // (k + 1)) % 5]
    it["u"] = u
    return it


# ---------------------------------------------------------------------------------------------------------------- margins
RELATIVE = {"t": 1e-30, "pdf_success": 1e-3, "phase_eval": 1e-3, "phase_pdf": 1e-3}  # quantity → floor of the denominator
CLASSES = ("edge", "random")  # the first N_EDGE items of a medium (random numbers at the edges: 1 - u / weight cancels), and the rest
N_EDGE = 64


def item_class(n=None):
    return (np.arange(N_ITEMS if n is None else n) >= N_EDGE).astype(int)
QUANTITIES = ("t", "pdf_success", "pdf_failure", "transmittance", "eval_transmittance", "wo", "phase_eval", "phase_pdf")


def difference(q, got, want):
    """|got - want| per item (the largest over the components), relative for the quantities that span decades; NaN where `want` is not finite"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got - want)
        if q in RELATIVE:
            d = d / np.maximum(np.abs(want), RELATIVE[q])
        d = np.where(np.isfinite(want), d, np.nan)
        d = np.where(np.isinf(want) & (got == want), 0.0, d)
    return d.reshape(d.shape[0], -1).max(axis=1) if d.ndim > 1 else d


def unsure(r64, items, margin_t):
    """items float64 cannot decide: the sampled distance within the margin of the length, u0 within float32's spacing of the sampling weight"""
    length = np.asarray(items["length"], np.float64)
    with np.errstate(all="ignore"):
        near_len = np.isfinite(r64["sampled"]) & np.isfinite(length) & (np.abs(r64["sampled"] - length) <= margin_t * np.maximum(length, r64["sampled"]))
    u0 = np.asarray(items["u"], np.float64)[:, 0]
    # (a weight of 0 leaves nothing to decide: no number lies below it, in any precision)
    near_w = (np.abs(u0 - r64["weight"]) <= 2.0 ** -23 * float(r64["weight"])) & (float(r64["weight"]) > 0)
    return near_len | near_w


def figures():
    """{class: {quantity: the largest float32 / float64 difference of the restatement over every medium's items of the class, the unsure
    ones left out}}"""
    fig = {c: {q: 0.0 for q in QUANTITIES} for c in CLASSES}
    for k, (_, medium) in enumerate(MEDIA):
        it = items_for(k, medium)
        r32, r64 = evaluate(medium, it, np.float32), evaluate(medium, it, np.float64)
        sure = ~unsure(r64, it, 8 * 1e-5) & (r32["success"] == r64["success"])
        for ci, c in enumerate(CLASSES):
            for q in QUANTITIES:
                d = difference(q, r32[q], r64[q])[sure & (item_class() == ci)]
                d = d[np.isfinite(d)]
                if d.size:
                    fig[c][q] = max(fig[c][q], float(d.max()))
    return fig


# what figures() gives for MEDIA / items_for (asserted equal, to two digits, in tests/test_media.py)
FIGURES = {"edge": {"t": 4.3e-06, "pdf_success": 3e-05, "pdf_failure": 8.7e-08, "transmittance": 3.9e-07, "eval_transmittance": 8.6e-08, "wo": 0.00091,
                    "phase_eval": 8.5e-05, "phase_pdf": 8.5e-05},
           "random": {"t": 0.00023, "pdf_success": 1.8e-05, "pdf_failure": 1.4e-07, "transmittance": 6.2e-07, "eval_transmittance": 1.1e-07, "wo": 2.7e-05,
                      "phase_eval": 0.00012, "phase_pdf": 0.00012}}
MARGIN = {c: {q: 8.0 * v for q, v in FIGURES[c].items()} for c in CLASSES}


def unsure_share():
    """the largest share of unsure items among the media (the GPU test allows 1 % per medium)"""
    worst = 0.0
    for k, (_, medium) in enumerate(MEDIA):
        it = items_for(k, medium)
        worst = max(worst, float(unsure(evaluate(medium, it, np.float64), it, max(MARGIN[c]["t"] for c in CLASSES)).mean()))
    return worst


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "practical-path-guiding_amd"))
    print({c: {q: float("%.2g" % v) for q, v in f.items()} for c, f in figures().items()}, "unsure share", unsure_share())
