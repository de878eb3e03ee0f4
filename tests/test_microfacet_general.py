"""The whole of Mitsuba's MicrofacetDistribution (alphaU / alphaV, beckmann / ggx / phong, sampling of all or of the visible normals):

  * a numpy restatement of the distribution, written from the formulas (Walter et al. 2007; Heitz and d'Eon 2014; Ashikhmin and Shirley
    2000), in a precision of the caller's choice, checked against itself: D integrates to one over projected solid angle, and the normals
    either sampler draws are distributed like its density.  The GPU tests (test_microfacet_general_gpu.py) hold the kernels to it;
  * both scene loaders accept such materials, emit equal bytes, and report Mitsuba's own errors.
"""
import os
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import mitsuba_xml

from test_bsdfs import sphere_grid, unit

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TYPES = ("beckmann", "ggx", "phong")
ALPHAS = ((0.25, 0.25), (0.05, 0.3), (0.3, 0.05), (0.6, 0.1))
WIS = {"normal": (0, 0, 1), "oblique": (0.6, 0.2, 0.5), "grazing": (-0.3, 0.9, 0.08), "from-below": (0.5, -0.3, -0.6)}  # test_bsdfs.py:98


# ------------------------------------------------------------------------------------------------ the restatement
def _erfinv(x, dt):
    """Giles' single-precision polynomial for erfinv, the one Mitsuba samples Beckmann slopes with"""
    w = -np.log((dt(1) - x) * (dt(1) + x))
    a = w - dt(2.5)
    p = dt(2.81022636e-08)
    for c in (3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087, -0.00125372503, -0.00417768164, 0.246640727, 1.50140941):
        p = dt(c) + p * a
    b = np.sqrt(np.maximum(w, dt(0))) - dt(3)
    q = dt(-0.000200214257)
    for c in (0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773, -0.0076224613, 0.00943887047, 1.00167406, 2.83297682):
        q = dt(c) + q * b
    return np.where(w < dt(5), p, q) * x


def _erf(x, dt):
    """Abramowitz and Stegun 7.1.26"""
    a1, a2, a3, a4, a5, p = (dt(v) for v in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429, 0.3275911))
    s = np.where(np.signbit(x), dt(-1), dt(1))
    x = np.abs(x)
    t = dt(1) / (dt(1) + p * x)
    return s * (dt(1) - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * np.exp(-x * x))


class Distribution:
    """D, G1 and the two samplers of one microfacet distribution, vectorised; every array and constant has dtype `dt`."""

    def __init__(self, kind, alpha_u, alpha_v, dt=np.float64):
        assert kind in TYPES
        self.kind, self.dt = kind, dt
        self.au, self.av = max(dt(alpha_u), dt(1e-4)), max(dt(alpha_v), dt(1e-4))
        self.pi = dt(np.pi)
        self.eu = max(dt(2) / (self.au * self.au) - dt(2), dt(0))  # Walter et al.: Phong exponent of a Beckmann roughness
        self.ev = max(dt(2) / (self.av * self.av) - dt(2), dt(0))
        self.iso = self.au == self.av

    def scaled(self, s):
        return Distribution(self.kind, self.au * self.dt(s), self.av * self.dt(s), self.dt)

    def _a(self, v):
        return np.asarray(v, self.dt).reshape(-1, 3)

    def D(self, m):
        dt = self.dt
        m = self._a(m)
        x, y, z = m[:, 0], m[:, 1], m[:, 2]
        with np.errstate(all="ignore"):
            c2 = z * z
            be = ((x * x) / (self.au * self.au) + (y * y) / (self.av * self.av)) / c2
            if self.kind == "beckmann":
                r = np.exp(-be) / (self.pi * self.au * self.av * c2 * c2)
            elif self.kind == "ggx":
                root = (dt(1) + be) * c2
                r = dt(1) / (self.pi * self.au * self.av * root * root)
            else:
                s2 = dt(1) - c2
                e = self.eu * (x * x / s2) + self.ev * (y * y / s2)
                e = np.where(s2 <= dt(0), self.eu, e) if not self.iso else np.full_like(z, self.eu)
                r = np.sqrt((self.eu + dt(2)) * (self.ev + dt(2))) / (dt(2) * self.pi) * np.power(np.maximum(z, dt(0)), e)
            r = np.where(r * z < dt(1e-20), dt(0), r)
        return np.where(z <= 0, dt(0), r).astype(dt)

    def G1(self, v, m):
        dt = self.dt
        v, m = self._a(v), self._a(m)
        z = v[:, 2]
        with np.errstate(all="ignore"):
            s2 = dt(1) - z * z
            tan = np.where(s2 <= 0, dt(0), np.abs(np.sqrt(np.maximum(s2, dt(0))) / z))
            if self.iso:
                alpha = np.full_like(z, self.au)
            else:  # the roughness projected on v's azimuth
                alpha = np.sqrt((v[:, 0] * v[:, 0] / s2) * self.au * self.au + (v[:, 1] * v[:, 1] / s2) * self.av * self.av)
                alpha = np.where(s2 <= 0, self.au, alpha)
            if self.kind == "ggx":
                root = alpha * tan
                g = dt(2) / (dt(1) + np.sqrt(dt(1) + root * root))
            else:  # Beckmann's rational fit, used for Phong too
                a = dt(1) / (alpha * tan)
                g = np.where(a >= dt(1.6), dt(1), (dt(3.535) * a + dt(2.181) * a * a) / (dt(1) + dt(2.276) * a + dt(2.577) * a * a))
            g = np.where(tan == 0, dt(1), g)
        return np.where((v * m).sum(1) * z <= 0, dt(0), g).astype(dt)

    def pdf_all(self, m):
        return self.D(m) * self._a(m)[:, 2]

    def pdf_visible(self, wi, m):
        wi, m = self._a(wi), self._a(m)
        with np.errstate(all="ignore"):
            r = self.G1(wi, m) * np.abs((wi * m).sum(1)) * self.D(m) / np.abs(wi[:, 2])
        return np.where(wi[:, 2] == 0, self.dt(0), r)

    def sample_all(self, u):
        """the normal and its density for u = (u.x, u.y) [n, 2]"""
        dt = self.dt
        u = np.asarray(u, dt).reshape(-1, 2)
        ux, uy = u[:, 0], u[:, 1]
        two_pi = dt(2) * self.pi
        with np.errstate(all="ignore"):
            if self.kind != "phong":
                if self.iso:
                    phi = two_pi * uy
                    a2 = np.full_like(ux, self.au * self.au)
                else:
                    phi = np.arctan(self.av / self.au * np.tan(self.pi + two_pi * uy)) + self.pi * np.floor(dt(2) * uy + dt(0.5))
                    cs, sn = np.cos(phi) / self.au, np.sin(phi) / self.av
                    a2 = dt(1) / (cs * cs + sn * sn)
                if self.kind == "beckmann":
                    t2 = a2 * -np.log(dt(1) - ux)
                    cz = dt(1) / np.sqrt(dt(1) + t2)
                    pdf = (dt(1) - ux) / (self.pi * self.au * self.av * cz * cz * cz)
                else:
                    t2 = a2 * ux / (dt(1) - ux)
                    cz = dt(1) / np.sqrt(dt(1) + t2)
                    tmp = dt(1) + t2 / a2
                    pdf = (dt(1) / self.pi) / (self.au * self.av * cz * cz * cz * tmp * tmp)
            else:
                if self.iso:
                    phi = two_pi * uy
                    e = np.full_like(ux, self.eu)
                else:  # Ashikhmin-Shirley: the first quadrant's azimuth, mirrored into the other three
                    q = np.minimum((uy * dt(4)).astype(np.int64), 3)
                    u1 = np.choose(q, [dt(4) * uy, dt(4) * (dt(0.5) - uy), dt(4) * (uy - dt(0.5)), dt(4) * (dt(1) - uy)])
                    p1 = np.arctan(np.sqrt((self.eu + dt(2)) / (self.ev + dt(2))) * np.tan(self.pi * u1 * dt(0.5)))
                    e = self.eu * np.cos(p1) ** 2 + self.ev * np.sin(p1) ** 2
                    phi = np.choose(q, [p1, self.pi - p1, p1 + self.pi, two_pi - p1])
                cz = np.power(ux, dt(1) / (e + dt(2)))
                pdf = np.sqrt((self.eu + dt(2)) * (self.ev + dt(2))) / two_pi * np.power(cz, e + dt(1))
            pdf = np.where(pdf < dt(1e-20), dt(0), pdf)
            sz = np.sqrt(np.maximum(dt(0), dt(1) - cz * cz))
        return np.stack([sz * np.cos(phi), sz * np.sin(phi), cz], 1).astype(dt), pdf.astype(dt)

    def _visible11(self, theta, ux, uy):
        """slopes of the visible normals of the unit-roughness surface seen from (sin theta, 0, cos theta): Heitz and d'Eon's supplement"""
        dt = self.dt
        two_pi = dt(2) * self.pi
        with np.errstate(all="ignore"):
            tan = np.tan(theta)
            if self.kind == "ggx":
                r0 = np.sqrt(np.maximum(dt(0), ux / (dt(1) - ux)))
                a = dt(1) / tan
                g1 = dt(2) / (dt(1) + np.sqrt(np.maximum(dt(0), dt(1) + dt(1) / (a * a))))
                A = dt(2) * ux / g1 - dt(1)
                A = np.where(np.abs(A) == 1, A - np.sign(A) * dt(1e-4), A)
                tmp = dt(1) / (A * A - dt(1))
                B = tan
                Dq = np.sqrt(np.maximum(dt(0), B * B * tmp * tmp - (A * A - B * B) * tmp))
                s1, s2 = B * tmp - Dq, B * tmp + Dq
                sx = np.where((A < 0) | (s2 > dt(1) / tan), s1, s2)
                S = np.where(uy > dt(0.5), dt(1), dt(-1))
                v = np.where(uy > dt(0.5), dt(2) * (uy - dt(0.5)), dt(2) * (dt(0.5) - uy))
                z = ((v * (v * (v * dt(-0.365728915865723) + dt(0.790235037209296)) - dt(0.424965825137544)) + dt(0.000152998850436920)) /
                     (v * (v * (v * (v * dt(0.169507819808272) - dt(0.397203533833404)) - dt(0.232500544458471)) + dt(1)) - dt(0.539825872510702)))
                sy = S * z * np.sqrt(dt(1) + sx * sx)
            else:
                r0 = np.sqrt(-np.log(dt(1) - ux))
                spi = dt(1) / np.sqrt(self.pi)
                cot = dt(1) / tan
                a = np.full_like(ux, dt(-1))
                c = _erf(cot, dt) + np.zeros_like(ux)
                sxm = np.maximum(ux, dt(1e-6))
                fit = dt(1) + theta * (dt(-0.876) + theta * (dt(0.4265) - dt(0.0594) * theta))
                b = c - (dt(1) + c) * np.power(dt(1) - sxm, fit)
                norm = dt(1) / (dt(1) + c + spi * tan * np.exp(-cot * cot))
                done = np.zeros(ux.shape, bool)
                for _ in range(9):  # Newton steps inside a shrinking bracket
                    b = np.where(~done & ~((b >= a) & (b <= c)), dt(0.5) * (a + c), b)
                    ie = _erfinv(b, dt)
                    value = norm * (dt(1) + b + spi * tan * np.exp(-ie * ie)) - sxm
                    deriv = norm * (dt(1) - ie * tan)
                    done = done | (np.abs(value) < dt(1e-5))
                    c = np.where(~done & (value > 0), b, c)
                    a = np.where(~done & ~(value > 0), b, a)
                    b = np.where(done, b, b - value / deriv)
                sx = _erfinv(b, dt)
                sy = _erfinv(dt(2) * np.maximum(uy, dt(1e-6)) - dt(1), dt)
            small = theta < dt(1e-4)  # normal incidence: the slope distribution itself
            sx = np.where(small, r0 * np.cos(two_pi * uy), sx)
            sy = np.where(small, r0 * np.sin(two_pi * uy), sy)
        return sx, sy

    def sample_visible(self, wi, u):
        dt = self.dt
        assert self.kind != "phong"
        u = np.asarray(u, dt).reshape(-1, 2)
        wi = np.broadcast_to(self._a(wi), (len(u), 3))
        s = np.stack([self.au * wi[:, 0], self.av * wi[:, 1], wi[:, 2]], 1)  # stretch
        s = s / np.sqrt((s * s).sum(1))[:, None]
        flat = s[:, 2] < dt(0.99999)
        theta = np.where(flat, np.arccos(np.clip(s[:, 2], -1, 1)), dt(0))
        phi = np.where(flat, np.arctan2(s[:, 1], s[:, 0]), dt(0))
        sx, sy = self._visible11(theta.astype(dt), u[:, 0], u[:, 1])
        rx = (np.cos(phi) * sx - np.sin(phi) * sy) * self.au  # rotate, unstretch
        ry = (np.sin(phi) * sx + np.cos(phi) * sy) * self.av
        n = dt(1) / np.sqrt(rx * rx + ry * ry + dt(1))
        return np.stack([-rx * n, -ry * n, n], 1).astype(dt)

    def sample(self, wi, u, sample_all):
        if sample_all:
            return self.sample_all(u)
        m = self.sample_visible(wi, u)
        return m, self.pdf_visible(np.broadcast_to(self._a(wi), m.shape), m)

    def pdf(self, wi, m, sample_all):
        return self.pdf_all(m) if sample_all else self.pdf_visible(wi, m)


def conductor_eval_pdf(distr, sample_all, wi, wo):
    """roughconductor with Fresnel = 1: f |cos theta_o| = D G / (4 cos theta_i), and the density of wo"""
    dt = distr.dt
    wi, wo = distr._a(wi), distr._a(wo)
    wi = np.broadcast_to(wi, wo.shape)
    h = wi + wo
    h = h / np.sqrt((h * h).sum(1))[:, None]
    with np.errstate(all="ignore"):
        f = distr.D(h) * distr.G1(wi, h) * distr.G1(wo, h) / (dt(4) * wi[:, 2])
        if sample_all:
            p = distr.pdf_all(h) / (dt(4) * np.abs((wo * h).sum(1)))
        else:
            p = distr.D(h) * distr.G1(wi, h) / (dt(4) * wi[:, 2])
    ok = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    return np.where(ok, f, dt(0)), np.where(ok, p, dt(0))


CASES = [(k, sa, a, w) for k in TYPES for sa in (False, True) for a in ALPHAS for w in WIS if not (k == "phong" and not sa)]
# (phong has no visible-normal sampler: the distribution switches it off itself, so "both samplers" is one for it)


def _id(c):
    return "%s-%s-%g-%g-%s" % (c[0], "all" if c[1] else "visible", c[2][0], c[2][1], c[3])


_grid = {}


def grid():
    if not _grid:
        d, dw, shape = sphere_grid()
        _grid["g"] = (d.astype(np.float64), dw, shape)
    return _grid["g"]


@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("alphas", ALPHAS, ids=["%g-%g" % a for a in ALPHAS])
def test_distribution_integrates_to_one(kind, alphas):
    d, dw, _ = grid()
    D = Distribution(kind, *alphas)
    total = float((D.D(d) * d[:, 2] * dw)[d[:, 2] > 0].sum())
    assert abs(total - 1) < 0.01, total


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_sampled_normals_follow_the_density(case):
    kind, sample_all, alphas, wname = case
    wi = unit(WIS[wname]).astype(np.float64)
    wi = wi * (1.0 if wi[2] >= 0 else -1.0)  # the plug-ins hand the distribution sign(cos theta_i) * wi
    D = Distribution(kind, *alphas)
    rng = np.random.RandomState(7)
    xy = rng.rand(400000, 2).astype(np.float32).astype(np.float64)
    m, pdf = D.sample(wi, xy, sample_all)
    assert np.all(np.isfinite(m)) and np.allclose((m * m).sum(1), 1, atol=1e-9)
    # the density the sampler reports is the density function's value
    ok = pdf > 0
    assert np.allclose(pdf[ok], D.pdf(np.broadcast_to(wi, m.shape), m, sample_all)[ok], rtol=1e-6, atol=1e-12)
    d, dw, shape = grid()
    pg = D.pdf(np.broadcast_to(wi, d.shape), d, sample_all)
    total = float((pg * dw).sum())
    assert abs(total - 1) < 0.01, total
    nb_t, nb_p = 18, 12
    H = (pg * dw).reshape(shape).reshape(nb_t, shape[0] // nb_t, nb_p, shape[1] // nb_p).sum((1, 3))
    it = np.clip((np.arccos(np.clip(m[:, 2], -1, 1)) / np.pi * nb_t).astype(int), 0, nb_t - 1)
    ip = np.clip(((np.arctan2(m[:, 1], m[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nb_p).astype(int), 0, nb_p - 1)
    cnt = np.zeros((nb_t, nb_p)); np.add.at(cnt, (it, ip), 1)
    emp = cnt / len(xy)
    big = H > 2e-3
    assert big.sum() >= 3
    assert np.allclose(emp[big], H[big], rtol=0.08, atol=2e-4), np.abs(emp[big] / H[big] - 1).max()


def test_phong_exponents_and_scaling():
    D = Distribution("phong", 0.2, 0.1)
    assert np.isclose(D.eu, 2 / 0.04 - 2) and np.isclose(D.ev, 2 / 0.01 - 2)
    assert Distribution("phong", 2.0, 2.0).eu == 0  # never negative
    S = D.scaled(1.1)
    assert np.isclose(S.au, 0.22) and np.isclose(S.eu, 2 / 0.22 ** 2 - 2)
    # with equal exponents the Ashikhmin-Shirley form is Phong's: (e + 2) / (2 pi) cos^e
    P = Distribution("phong", 0.3, 0.3)
    m = unit((0.2, -0.1, 0.9)).astype(np.float64)
    assert np.isclose(P.D(m)[0], (P.eu + 2) / (2 * np.pi) * m[2] ** P.eu)


# ------------------------------------------------------------------------------------------------ the loaders
HEAD = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="4"/> </integrator>
  <sensor type="perspective"> <float name="fov" value="45"/>
    <transform name="toWorld"> <lookAt origin="0, 1, -5" target="0, 1, 0" up="0, 1, 0"/> </transform>
    <film type="hdrfilm"> <integer name="width" value="8"/> <integer name="height" value="6"/> <rfilter type="box"/> </film> </sensor>
  <shape type="rectangle"> <emitter type="area"> <rgb name="radiance" value="1, 1, 1"/> </emitter> </shape>
  %s
</scene>
"""
QUAD_VT = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3\nf 1/1 3/3 4/4\n"
QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3\nf 1 3 4\n"
MESH_VT = '<shape type="obj"> <string name="filename" value="quad_vt.obj"/> %s </shape>'
MESH = '<shape type="obj"> <string name="filename" value="quad.obj"/> %s </shape>'
SPHERE = '<shape type="sphere"> %s </shape>'
NONE = '<string name="material" value="none"/>'
REF_DATA = os.environ.get("PPG_MITSUBA_DATA", "/root/reference/mitsuba/data")
BIN = os.path.join(os.path.dirname(__file__), "..", "practical-path-guiding_amd", "bin", "ppg_render")


def _scene(tmp_path, body):
    (tmp_path / "quad_vt.obj").write_text(QUAD_VT)
    (tmp_path / "quad.obj").write_text(QUAD)
    p = tmp_path / "s.xml"
    p.write_text(HEAD % body)
    return str(p)


def _python(tmp_path, body, **kw):
    desc, _, info = ppg_host.load_scene(_scene(tmp_path, body), **kw)
    assert not info["warnings"]
    return desc


def _cpp(tmp_path, body, *extra):
    if not os.path.exists(BIN):
        import sys
        subprocess.check_call([sys.executable, os.path.join(os.path.dirname(__file__), "..", "__graft_entry__.py")])
    out = str(tmp_path / "cpp.ppgs")
    r = subprocess.run([BIN, "--ppgs", out, "-q", *extra, _scene(tmp_path, body)], capture_output=True, text=True)
    return r, (open(out, "rb").read() if r.returncode == 0 else None)


def _entries(desc):
    """the bytes of the scene's ppg_material records and of its microfacet list"""
    from ppg_host.bindings import Material, Microfacet
    return b"".join(bytes(Material.from_dict(m)) for m in desc.materials), b"".join(bytes(Microfacet.from_dict(m)) for m in desc.materials)


ACCEPTED = {
    "a-aniso-ggx": ('<bsdf type="roughconductor"> %s <string name="distribution" value="ggx"/> <float name="alphaU" value="0.05"/> <float name="alphaV" value="0.3"/> </bsdf>' % NONE,
                    dict(alpha=0.05, alpha_v=0.3)),
    "b-beckmann-all": ('<bsdf type="roughdielectric"> <string name="distribution" value="beckmann"/> <boolean name="sampleVisible" value="false"/> </bsdf>',
                       dict(alpha=0.1, distribution="beckmann", sample_visible=False)),
    "equal-alphas": ('<bsdf type="roughconductor"> %s <string name="distribution" value="ggx"/> <float name="alphaU" value="0.2"/> <float name="alphaV" value="0.2"/> </bsdf>' % NONE,
                     dict(alpha=0.2, alpha_v=0.2)),
}


@pytest.mark.parametrize("where", ["sphere", "mesh-vt"])
@pytest.mark.parametrize("name", list(ACCEPTED))
def test_loaders_accept_and_agree(tmp_path, name, where):
    """on a mesh that carries `vt` and on an analytic sphere (which spans its own tangent frame) both loaders make the same ppg_material
    records, the same ppg_microfacet list and — for the anisotropic BSDF on the mesh — the same texture coordinates, byte for byte"""
    from ppg_host.bindings import Microfacet
    bsdf, want = ACCEPTED[name]
    body = (SPHERE if where == "sphere" else MESH_VT) % bsdf
    desc = _python(tmp_path, body)
    m = desc.materials[-1]
    for k, v in want.items():
        assert m[k] == v or (isinstance(v, float) and np.isclose(m[k], v)), (k, m)
    g = Microfacet.from_dict(m)
    assert g.general == 1 and g.distribution == 0 and g.sample_all == (0 if want.get("sample_visible", True) else 1)
    assert np.float32(g.alpha_v) == np.float32(want.get("alpha_v", want["alpha"]))
    assert (desc.texcoords is not None) == (where != "sphere" and name == "a-aniso-ggx")
    mats, mfd = _entries(desc)
    r, flat = _cpp(tmp_path, body)
    assert r.returncode == 0, r.stderr
    mine = open(_save(desc, tmp_path), "rb").read()
    assert np.array_equal(np.frombuffer(flat, np.uint32, 6, 4), np.frombuffer(mine, np.uint32, 6, 4)) and int(np.frombuffer(flat, np.uint32, 6, 4)[5]) & 2048
    assert _material_records(flat) == _material_records(mine) == mats
    assert flat.endswith(mfd) and mine.endswith(mfd)        # the microfacet block is the file's last
    if desc.texcoords is not None:
        uv = np.ascontiguousarray(desc.texcoords, np.float32).tobytes()
        assert flat.count(uv) == 1 and mine.count(uv) == 1
    # ... and the flat file gives the material dicts back
    assert _entries(ppg_host.load_scene_file(_save(desc, tmp_path))) == (mats, mfd)


def _material_records(flat):
    """the bytes of the ppg_material records of a flat scene file"""
    nv, nt, nm, ne, has_n, _ = (int(v) for v in np.frombuffer(flat, np.uint32, 6, 4))
    off = 28 + nv * 12 * (2 if has_n else 1) + nt * 20
    return flat[off:off + 80 * nm]


def _save(desc, tmp_path):
    p = str(tmp_path / "py.ppgs")
    ppg_host.save_scene(desc, p)
    return p


@pytest.mark.skipif(not os.path.exists(os.path.join(REF_DATA, "microfacet", "phong.dat")), reason="needs Mitsuba's data/microfacet/phong.dat")
def test_roughplastic_phong_takes_its_slice_from_the_phong_table(tmp_path):
    bsdf = '<bsdf type="roughplastic"> <string name="distribution" value="phong"/> <float name="alpha" value="0.2"/> </bsdf>'
    desc = _python(tmp_path, SPHERE % bsdf, data_dir=REF_DATA)
    g = np.load(os.path.join(GOLDEN, "rtrans_slices_phong.npz"))
    assert g["slice0"].shape == (101,) and np.array_equal(desc.rtrans[0], g["slice0"])
    m = desc.materials[desc.spheres[0]["material"]]
    assert m["distribution"] == "phong" and m["type"] == 9
    r, flat = _cpp(tmp_path, SPHERE % bsdf, "--data-dir", REF_DATA)
    assert r.returncode == 0, r.stderr
    mine = open(_save(desc, tmp_path), "rb").read()
    assert _material_records(flat) == _material_records(mine) and flat.endswith(_entries(desc)[1])
    assert flat.count(g["slice0"].tobytes()) == 1  # the same slice, bit for bit (host/rough_transmittance.h)


def test_python_loader_reads_bitmaps_on_both_alphas(tmp_path):
    from ppg_host import imageio
    rng = np.random.RandomState(2)
    for n in ("u", "v"):
        imageio.write_pfm(str(tmp_path / ("a%s.pfm" % n)), (rng.rand(4, 4, 3) * 0.3 + 0.05).astype(np.float32))
    tex = '<texture name="alpha%s" type="bitmap"> <string name="filename" value="a%s.pfm"/> <float name="gamma" value="1"/> </texture>'
    desc = _python(tmp_path, MESH_VT % ('<bsdf type="roughconductor"> %s %s %s </bsdf>' % (NONE, tex % ("U", "u"), tex % ("V", "v"))))
    m = desc.materials[-1]
    assert m["alpha_texture"] == 0 and m["alpha_v_texture"] == 1 and len(desc.textures) == 2 and desc.texcoords is not None
    assert np.isclose(m["alpha"], np.mean(desc.textures[0]["rgb"])) and np.isclose(m["alpha_v"], np.mean(desc.textures[1]["rgb"]))


REFUSED = {
    "alpha-and-alphaU": (SPHERE % ('<bsdf type="roughconductor"> %s <float name="alpha" value="0.1"/> <float name="alphaU" value="0.2"/> </bsdf>' % NONE),
                         "please specify either 'alpha' or 'alphaU'/'alphaV'"),
    "alphaU-alone": (SPHERE % ('<bsdf type="roughdielectric"> <float name="alphaU" value="0.2"/> </bsdf>'), "both 'alphaU' and 'alphaV' must be specified"),
    "roughplastic-aniso": (SPHERE % '<bsdf type="roughplastic"> <float name="alphaU" value="0.2"/> <float name="alphaV" value="0.3"/> </bsdf>',
                           "does not support anisotropic microfacet distributions"),
    "phong-on-roughconductor": (SPHERE % ('<bsdf type="roughconductor"> %s <string name="distribution" value="phong"/> </bsdf>' % NONE),
                                "is not supported by the scene loaders on this plug-in"),
    "aniso-without-vt": (MESH % ('<bsdf type="roughconductor"> %s <float name="alphaU" value="0.05"/> <float name="alphaV" value="0.3"/> </bsdf>' % NONE),
                         "texture coordinates are required to generate tangent vectors"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_loaders_refuse_with_mitsubas_words(tmp_path, name):
    body, needle = REFUSED[name]
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _python(tmp_path, body)
    assert needle in str(ei.value)
    r, _ = _cpp(tmp_path, body)
    assert r.returncode != 0 and needle in r.stderr, r.stderr


def test_xml_writer_round_trip(tmp_path):
    from ppg_host.bindings import Material, Microfacet
    scene = ppg_host.cbox_scene(8, 8)
    scene.materials = list(scene.materials) + [
        dict(type="roughconductor", alpha=0.2, alpha_v=0.05, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.1), reflectance=(1, 1, 1)),
        dict(type="roughdielectric", alpha=0.25, eta=1.5, reflectance=(1, 1, 1), specular=(0.9, 0.95, 1.0), distribution="beckmann", sample_visible=False)]
    scene.spheres = [dict(center=(100.0, 100.0, 100.0), radius=20.0, material=5, emitter=-1)]  # (a sphere spans its own tangent frame)
    tm = scene.tri_material.copy(); tm[2] = 6; scene.tri_material = tm
    path = ppg_host.save_scene_xml(scene, dict(budgetType="spp", budget=8.0), str(tmp_path))
    back, _, info = ppg_host.load_scene(path)
    assert not info["warnings"]
    rec = lambda m: bytes(Material.from_dict(m)) + bytes(Microfacet.from_dict(m))  # noqa: E731
    assert rec(back.materials[back.spheres[0]["material"]]) == rec(scene.materials[5])
    assert rec(scene.materials[6]) in {rec(back.materials[int(t)]) for t in back.tri_material}
    # phong is written by name (the loaders read it back on roughplastic only)
    scene.materials[5] = dict(scene.materials[5], alpha_v=0.2, distribution="phong")
    text = open(ppg_host.save_scene_xml(scene, dict(budgetType="spp", budget=8.0), str(tmp_path / "p"))).read()
    assert '<string name="distribution" value="phong"/><float name="alphaU" value="0.2' in text
