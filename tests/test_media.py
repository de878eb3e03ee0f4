"""Homogeneous participating media without a GPU (include/ppg.h ppg_set_media):
  * the numpy restatement (tests/medium_ref.py) against closed forms, and its float32 / float64 figures;
  * the Python loader: media on the sensor and on shapes, inline and by reference, and every refusal by its message;
  * the bindings: struct sizes, the packing of a medium dict, the refusals for the oracle library and the scene writers;
  * ppg_set_scene's validation and derived tables through the host build stage (tests/media_build_check.hip, no device).
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import bindings as B
from ppg_host import mitsuba_xml
from conftest import ROOT, ORACLE_SO

import medium_ref as R

SceneError = mitsuba_xml.SceneError
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
f64 = np.float64


# ------------------------------------------------------------------------------------------------ 1. the restatement
def test_figures_are_the_measured_ones_and_few_items_are_unsure():
    fig = R.figures()
    for c in R.CLASSES:
        for q in R.QUANTITIES:
            assert float("%.2g" % fig[c][q]) == R.FIGURES[c][q], (c, q, fig[c][q])
    assert R.unsure_share() < 0.01


def _gauss_sphere(n=400):
    """Gauss-Legendre in cos(theta) x uniform phi: (directions [n * 16, 3], weights)"""
    x, w = np.polynomial.legendre.leggauss(n)
    phi = (np.arange(16) + 0.5) * (2 * np.pi / 16)
    s = np.sqrt(1 - x * x)
    d = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(x, np.ones(16))], -1).reshape(-1, 3)
    return d, np.repeat(w, 16) * (2 * np.pi / 16)


@pytest.mark.parametrize("g", [None, -0.9, 0.0, 1e-5, 0.3, 0.95])
def test_phase_functions_integrate_to_one_with_mean_cosine_g(g):
    D = R.derive(dict(sigma_a=1.0, sigma_s=1.0, **R._phase(g)), f64)
    wo, w = _gauss_sphere()
    wi = np.tile([0.0, 0.0, 1.0], (len(wo), 1))
    val = R.phase_eval(D, wi, wo)
    assert abs(np.sum(val * w) - 1) < 1e-9
    # wi points back along the ray: the mean cosine of the scattering angle, between -wi and wo, is g
    assert abs(np.sum(val * w * -wo[:, 2]) - (0.0 if g is None else float(np.float32(g)))) < 1e-9


@pytest.mark.parametrize("g", [None, -0.9, 1e-5, 0.3, 0.95])
def test_phase_sampling_follows_its_density(g):
    """the sampled directions are unit vectors, the returned density is the phase function's value there, and the sampled cosine's
    distribution is the density's: E[cos] = g by a midpoint rule over the first random number"""
    D = R.derive(dict(sigma_a=1.0, sigma_s=1.0, **R._phase(g)), f64)
    n = 20000
    sx = (np.arange(n) + 0.5) / n
    sy = np.full(n, 0.3)
    rng = np.random.default_rng(3)
    wi = rng.normal(size=(n, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo, pdf = R.phase_sample(D, wi, sx if g is not None else sy, sy if g is not None else sx)
    assert np.allclose(np.linalg.norm(wo, axis=1), 1, atol=1e-12)
    assert np.allclose(pdf, R.phase_eval(D, wi, wo), rtol=1e-12)
    cos = np.sum(-wi * wo, axis=1) if g is not None else wo[:, 2]
    # (below Epsilon hg samples the uniform sphere, hg.cpp:79-80, although its density keeps its — negligible — slope)
    assert abs(cos.mean() - (0.0 if g is None or abs(g) < R.EPSILON else float(np.float32(g)))) < 1e-6


@pytest.mark.parametrize("name,medium", R.MEDIA, ids=[m[0] for m in R.MEDIA])
def test_pdf_success_integrates_to_weight_times_one_minus_the_exponential(name, medium):
    """over [0, d] the density of a medium event integrates to samplingWeight * (1 - pdfFailure_exp(d)), pdfFailure_exp the strategy's
    exponential part: pdfFailure(d) = w * pdfFailure_exp(d) + (1 - w)"""
    D = R.derive(medium, f64)
    d = 1.7 / max(float(D["sigma_t"].max()), 1e-3)
    x, w = np.polynomial.legendre.leggauss(200)
    t = 0.5 * d * (x + 1)
    # (u0 = 2: no distance is sampled, every item fails at its length t and reports the densities there)
    r = R.sample_distance(D, t, np.full_like(t, 2.0), np.zeros_like(t), np.tile([0.0, 0.0, 1.0], (len(t), 1)))
    integral = np.sum(r["pdf_success"] * w) * 0.5 * d
    at_d = R.sample_distance(D, np.array([d]), np.array([2.0]), np.array([0.0]), np.array([[0.0, 0.0, 1.0]]))
    failure = float(at_d["pdf_failure"][0])
    assert abs(integral - (1 - failure)) < 1e-10  # = weight * (1 - pdfFailure_exp)


def test_sampled_distances_follow_the_density():
    """inverting the exponential: the share of events before d is weight * (1 - exp(-density d)) (single strategy)"""
    medium = dict(sigma_a=(0.3, 0.2, 0.1), sigma_s=(3.0, 2.0, 1.0), strategy="single")
    D = R.derive(medium, f64)
    n = 100000
    u0 = (np.arange(n) + 0.5) / n
    d = 0.8
    r = R.sample_distance(D, np.full(n, d), u0, np.zeros(n), np.tile([0.0, 0.0, 1.0], (n, 1)))
    assert abs(r["success"].mean() - float(D["weight"]) * (1 - np.exp(-float(D["density"]) * d))) < 2e-5
    assert float(D["density"]) == float(np.float32(0.1) + np.float32(1.0))


def test_rules_of_a_channel_without_extinction():
    D = R.derive(dict(sigma_a=(0.5, 0.0, 0.25), sigma_s=(1.0, 0.0, 2.0)), f64)
    # the default sampling weight looks at the channels that extinguish only: max(1 / 1.5, 2 / 2.25)
    assert abs(float(D["weight"]) - 2.0 / 2.25) < 1e-7
    tr = R.eval_transmittance(D, np.array([0.0, 1.0, np.inf]))
    assert np.all(tr[:, 1] == 1.0) and np.all(tr[2, [0, 2]] == 0.0) and abs(tr[1, 0] - np.exp(-1.5)) < 1e-12
    # sampleDistance multiplies without that rule: 0 * inf = NaN over an infinite segment (the densities of `balance` sum it in; in
    # Spectrum::max() it loses against the first channel's 0, so the "below 1e-20" rule zeroes the transmittance), 1 over a finite one
    r = R.sample_distance(D, np.array([1.0, np.inf]), np.array([2.0, 2.0]), np.zeros(2), np.tile([0.0, 0.0, 1.0], (2, 1)))
    assert r["transmittance"][0, 1] == 1.0 and (r["transmittance"][1] == 0).all() and np.isnan(r["pdf_failure"][1]) and not r["success"].any()
    # ... and where the FIRST channel is the one without extinction, the NaN wins and stays
    D0 = R.derive(dict(sigma_a=(0.0, 0.5, 0.5), sigma_s=(0.0, 1.0, 2.0), strategy="single", channel=1), f64)
    r0 = R.sample_distance(D0, np.array([np.inf]), np.array([2.0]), np.zeros(1), np.array([[0.0, 0.0, 1.0]]))
    assert np.isnan(r0["transmittance"][0, 0]) and (r0["transmittance"][0, 1:] == 0).all() and r0["pdf_failure"][0] == 1 - float(D0["weight"])
    # a pure absorber never scatters; a medium that scatters a little still gets half of the samples
    assert float(R.derive(dict(sigma_a=(1.0, 2.0, 3.0), sigma_s=0.0), f64)["weight"]) == 0.0
    assert float(R.derive(dict(sigma_a=9.0, sigma_s=1.0), f64)["weight"]) == 0.5
    assert float(R.derive(dict(sigma_t=(2.0, 3.0, 4.0), albedo=1.0, scale=0.5), f64)["weight"]) == 1.0


# ------------------------------------------------------------------------------------------------ 2. the loader
XML = """<scene version="0.5.0">
  <integrator type="guided_path"/>
  <sensor type="perspective"> <float name="fov" value="40"/> %(sensor)s
    <film type="hdrfilm"> <integer name="width" value="8"/> <integer name="height" value="8"/> <rfilter type="box"/> </film> </sensor>
  %(top)s
  %(shapes)s
  <shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1"/> </emitter> </shape>
</scene>
"""
FOG = '<medium type="homogeneous" %s> <rgb name="sigmaA" value="0.1, 0.2, 0.3"/> <rgb name="sigmaS" value="1, 2, 3"/> %s </medium>'


def _load(tmp_path, sensor="", top="", shapes="", strict=True):
    p = tmp_path / "s.xml"
    p.write_text(XML % dict(sensor=sensor, top=top, shapes=shapes))
    desc, _, info = ppg_host.load_scene(str(p), strict=strict)
    return desc, info


def test_fog_on_the_sensor(tmp_path):
    desc, info = _load(tmp_path, sensor=FOG % ("", '<phase type="hg"> <float name="g" value="0.5"/> </phase>'))
    assert not info["warnings"] and desc.camera_medium == 1 and desc.tri_media is None and desc.sphere_media is None and desc.shape_media is None
    assert len(desc.media) == 1 and sorted(desc.media[0]) == ["g", "phase", "scale", "sigma_a", "sigma_s", "strategy"]
    assert {k: desc.media[0][k] for k in ("g", "phase", "scale", "strategy")} == dict(scale=1.0, strategy="balance", phase="hg", g=0.5)
    for k, v in dict(sigma_a=(0.1, 0.2, 0.3), sigma_s=(1.0, 2.0, 3.0)).items():
        assert np.allclose(desc.media[0][k], v)
    # by reference, and the default hg asymmetry
    desc, _ = _load(tmp_path, sensor='<ref id="fog"/>', top=FOG % ('id="fog"', '<phase type="hg"/>'))
    assert desc.camera_medium == 1 and desc.media[0]["g"] == 0.8 and len(desc.media) == 1


def test_interior_on_a_cube_with_null_and_on_a_sphere_with_dielectric(tmp_path):
    shapes = ('<shape type="cube"> <bsdf type="null"/> ' + FOG % ('name="interior"', "") + ' </shape>'
              '<shape type="sphere"> <bsdf type="dielectric"/> ' + FOG % ('name="interior"', "") + FOG % ('name="exterior"', '<phase type="isotropic"/>') + ' </shape>'
              '<shape type="disk"> <ref name="exterior" id="smoke"/> </shape>')
    desc, info = _load(tmp_path, top=FOG % ('id="smoke"', ""), shapes=shapes)
    assert not info["warnings"] and len(desc.media) == 4 and desc.camera_medium == 0
    words = np.asarray(desc.tri_media)
    assert len(words) == desc.n_triangles and (words[:12] == B.media_word(interior=1)).all() and (words[12:] == 0).all()
    assert list(desc.sphere_media) == [B.media_word(interior=2, exterior=3)] and list(desc.shape_media) == [B.media_word(exterior=0)]
    assert B.media_word(interior=2, exterior=3) == 3 | (4 << 16) and B.media_word() == 0


def test_a_ref_shared_by_two_shapes(tmp_path):
    shapes = ('<shape type="cube"> <bsdf type="null"/> <ref name="interior" id="wax"/> </shape>'
              '<shape type="rectangle"> <bsdf type="null"/> <ref name="interior" id="wax"/> <ref name="exterior" id="fog"/> </shape>')
    desc, _ = _load(tmp_path, top=FOG % ('id="fog"', "") + FOG % ('id="wax"', ""), shapes=shapes)
    words = np.asarray(desc.tri_media)
    assert len(desc.media) == 2 and (words[:12] == B.media_word(interior=1)).all() and (words[12:14] == B.media_word(interior=1, exterior=0)).all()
    assert (words[14:] == 0).all()


def test_sigma_t_albedo_and_scale(tmp_path):
    medium = ('<medium type="homogeneous" name="interior"> <rgb name="sigmaT" value="2, 4, 8"/> <rgb name="albedo" value="0.5, 0.25, 1"/> <float name="scale" value="0.5"/>'
              ' <string name="strategy" value="single"/> <integer name="channel" value="2"/> <float name="mediumSamplingWeight" value="0.25"/> </medium>')
    desc, _ = _load(tmp_path, shapes='<shape type="cube"> <bsdf type="null"/> %s </shape>' % medium)
    m = B.Medium.from_dict(desc.media[0])
    assert list(m.sigma_s) == [0.5, 0.5, 4.0] and list(m.sigma_a) == [0.5, 1.5, 0.0]
    assert (m.strategy, m.channel, m.sampling_weight, m.phase) == (1, 2, 0.25, 0)
    manual = '<medium type="homogeneous" name="interior"> <rgb name="sigmaA" value="1"/> <rgb name="sigmaS" value="1"/> <string name="strategy" value="manual"/> <float name="samplingDensity" value="3"/> </medium>'
    desc, _ = _load(tmp_path, shapes='<shape type="cube"> <bsdf type="null"/> %s </shape>' % manual)
    m = B.Medium.from_dict(desc.media[0])
    assert (m.strategy, m.sampling_density, m.sampling_weight, m.channel) == (2, 3.0, -1.0, -1)


def _medium(body, attrs='name="interior"', kind="homogeneous"):
    return '<shape type="cube"> <bsdf type="null"/> <medium type="%s" %s> %s </medium> </shape>' % (kind, attrs, body)


AS = '<rgb name="sigmaA" value="1"/> <rgb name="sigmaS" value="1"/>'
REFUSALS = [
    ("heterogeneous", dict(shapes=_medium(AS, kind="heterogeneous")), "medium type 'heterogeneous' is not supported (homogeneous media only)"),
    ("maximum", dict(shapes=_medium(AS + '<string name="strategy" value="maximum"/>')), "strategy 'maximum' is not supported (balance, single, manual)"),
    ("unknown strategy", dict(shapes=_medium(AS + '<string name="strategy" value="best"/>')), "Specified an unknown sampling strategy ('best')"),
    ("monochromatic", dict(shapes=_medium(AS + '<string name="strategy" value="single"/> <boolean name="monochromatic" value="true"/>')), "'monochromatic' is not supported"),
    ("material preset", dict(shapes=_medium('<string name="material" value="Skin1"/>')), "the 'material' presets ('Skin1') are not supported"),
    ("sigmaA alone", dict(shapes=_medium('<rgb name="sigmaA" value="1"/>')), "state both sigmaA and sigmaS, or both sigmaT and albedo"),
    ("sigmaT alone", dict(shapes=_medium('<rgb name="sigmaT" value="1"/>')), "state both sigmaA and sigmaS, or both sigmaT and albedo"),
    ("nothing stated", dict(shapes=_medium("")), "state both sigmaA and sigmaS, or both sigmaT and albedo"),
    ("both pairs", dict(shapes=_medium(AS + '<rgb name="sigmaT" value="1"/>')), "please provide *either* sigmaA & sigmaS *or* sigmaT & albedo"),
    ("microflake", dict(shapes=_medium(AS + '<phase type="microflake"/>')), "phase function type 'microflake' is not supported (isotropic, hg)"),
    ("hg g", dict(shapes=_medium(AS + '<phase type="hg"> <float name="g" value="1"/> </phase>')), "The asymmetry parameter must lie in the interval (-1, 1)!"),
    ("manual without density", dict(shapes=_medium(AS + '<string name="strategy" value="manual"/>')), "strategy 'manual' needs 'samplingDensity'"),
    ("channel", dict(shapes=_medium(AS + '<string name="strategy" value="single"/> <integer name="channel" value="3"/>')), "channel must be 0, 1 or 2"),
    ("side name", dict(shapes=_medium(AS, attrs='name="inside"')), "a medium on a shape must be named 'interior' or 'exterior' (got 'inside')"),
    ("dangling ref", dict(shapes='<shape type="cube"> <ref name="interior" id="nowhere"/> </shape>'), "<ref id='nowhere'>: no such medium"),
    ("environment emitter", dict(top='<emitter type="constant"> %s </emitter>' % (FOG % ("", ""))), "a <medium> inside an emitter ('constant') is not supported"),
    ("delta emitter", dict(top=FOG % ('id="fog"', "") + '<emitter type="point"> <ref id="fog"/> <rgb name="intensity" value="1"/> </emitter>'),
     "a <medium> inside an emitter ('point') is not supported"),
    ("subsurface", dict(shapes='<shape type="cube"> <subsurface type="dipole"/> </shape>'), "subsurface plug-ins (<subsurface type='dipole'>) are not supported"),
]


@pytest.mark.parametrize("name,where,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_loader_refuses_by_name(tmp_path, name, where, message):
    with pytest.raises(SceneError) as err:
        _load(tmp_path, **where)
    assert message in str(err.value)


def test_a_lenient_load_drops_what_it_cannot_render_with_a_warning(tmp_path):
    shapes = (_medium(AS, kind="heterogeneous") + _medium(AS + '<string name="strategy" value="maximum"/>') + _medium(AS)
              + '<shape type="cube"> <subsurface type="dipole"/> <ref name="interior" id="het"/> </shape>')
    top = '<medium type="heterogeneous" id="het"/> <emitter type="constant"> %s </emitter>' % (FOG % ("", ""))
    desc, info = _load(tmp_path, sensor='<ref id="het"/>', top=top, shapes=shapes, strict=False)
    assert len(desc.media) == 1 and desc.camera_medium == 0
    words = np.asarray(desc.tri_media)
    assert (words[:24] == 0).all() and (words[24:36] == B.media_word(interior=0)).all() and (words[36:] == 0).all()
    w = "\n".join(info["warnings"])
    for part in ("medium dropped (id 'het'): medium type 'heterogeneous'", "medium dropped (interior of a cube shape)", "strategy 'maximum' is not supported",
                 "medium inside emitter 'constant' dropped", "subsurface 'dipole' on a shape dropped"):
        assert part in w, part
    assert desc.environment is not None


# ------------------------------------------------------------------------------------------------ 3. the bindings
def test_struct_sizes_and_packing():
    assert ctypes.sizeof(B.Medium) == 64 and ctypes.sizeof(B.Media) == 56
    assert ctypes.sizeof(B.DebugMediumItem) == 36 == B.DEBUG_MEDIUM_ITEM_DTYPE.itemsize == R.ITEM_DTYPE.itemsize
    assert ctypes.sizeof(B.DebugMediumOut) == 60 == B.DEBUG_MEDIUM_OUT_DTYPE.itemsize
    assert B.Medium.sigma_s.offset == 12 and B.Medium.strategy.offset == 24 and B.Medium.phase.offset == 40 and B.Medium._reserved.offset == 48
    assert B.Media.media.offset == 8 and B.Media.n_tri_media.offset == 16 and B.Media.tri_media.offset == 32 and B.Media.shape_media.offset == 48
    m = B.Medium.from_dict(dict(sigma_t=(2.0, 4.0, 8.0), albedo=(0.5, 0.25, 1.0), scale=0.5, strategy="manual", sampling_density=2.0, phase="hg", g=-0.3))
    assert list(m.sigma_a) == [0.5, 1.5, 0.0] and list(m.sigma_s) == [0.5, 0.5, 4.0] and (m.strategy, m.phase, m.channel) == (2, 1, -1)
    assert m.sampling_weight == -1.0 and abs(m.g + 0.3) < 1e-7 and list(m._reserved) == [0, 0, 0, 0]
    for bad in (dict(sigma_a=1.0), dict(sigma_t=1.0), dict(sigma_a=1.0, sigma_s=1.0, albedo=0.5), {}):
        with pytest.raises(ValueError, match="state sigma_a and sigma_s, or sigma_t and albedo"):
            B.Medium.from_dict(bad)


def _fog_box():
    desc = ppg_host.cbox_scene(8, 8)
    desc.media = [dict(sigma_a=0.1, sigma_s=0.2)]
    desc.camera_medium = 1
    return desc


def test_the_oracle_library_refuses_media(oracle_lib):
    e = ppg_host.Engine(ORACLE_SO, "ppgo_", budgetType="spp", budget=4)
    with pytest.raises(NotImplementedError, match="ppgo_: participating media are not implemented here"):
        e.set_scene(_fog_box())
    with pytest.raises(NotImplementedError, match="participating media"):
        e.set_media([dict(sigma_a=1.0, sigma_s=1.0)])
    e.set_scene(ppg_host.cbox_scene(8, 8))  # (and is none the worse for it)
    e.close()


def test_the_scene_writers_refuse_media(tmp_path):
    with pytest.raises(NotImplementedError, match=r"save_scene: participating media \(SceneDesc.media\) are not part of the .ppgs container"):
        ppg_host.save_scene(_fog_box(), str(tmp_path / "fog.ppgs"))
    with pytest.raises(NotImplementedError, match="save_scene_xml: participating media"):
        ppg_host.save_scene_xml(_fog_box(), {}, str(tmp_path))


CPP_PLAIN = '<shape type="cube"> <bsdf type="null"/> </shape> <shape type="sphere"> <bsdf type="dielectric"/> </shape>'
CPP_MEDIA = {  # what the C++ loader (host/scene_xml.h) does not offer, each on the scene CPP_PLAIN
    "medium on a shape": '<shape type="cube"> <bsdf type="null"/> %s </shape> <shape type="sphere"> <bsdf type="dielectric"/> </shape>' % (FOG % ('name="interior"', "")),
    "ref to a medium": ('%s <shape type="cube"> <bsdf type="null"/> <ref name="interior" id="fog"/> </shape>'
                        ' <shape type="sphere"> <bsdf type="dielectric"/> <ref name="exterior" id="fog"/> </shape>' % (FOG % ('id="fog"', ""))),
    "subsurface": '<shape type="cube"> <bsdf type="null"/> <subsurface type="dipole"/> </shape> <shape type="sphere"> <bsdf type="dielectric"/> </shape>',
}


@pytest.mark.parametrize("name", sorted(CPP_MEDIA))
def test_the_cpp_loader_refuses_media_by_name_and_a_lenient_load_drops_them(tmp_path, name):
    """`ppg_render --ppgs` (host/scene_xml.h) on a scene with a <medium> on a shape, a <ref name="interior">, a <subsurface>: a strict load
    fails and names what it is; a lenient load warns, and writes, byte for byte, the .ppgs of the scene without them"""
    from test_microfacet_general import BIN, _cpp, _scene
    body = CPP_MEDIA[name]
    r, flat = _cpp(tmp_path, body)
    assert r.returncode != 0 and flat is None
    want = ("subsurface plug-ins (<subsurface>) are not supported" if name == "subsurface" else
            "participating media (<medium>) are not offered by this loader: load the scene with the Python loader (ppg_host.mitsuba_xml)")
    assert want in r.stderr + r.stdout
    plain, flat_plain = _cpp(tmp_path, CPP_PLAIN)
    assert plain.returncode == 0, plain.stderr
    out = str(tmp_path / "lenient.ppgs")
    r = subprocess.run([BIN, "--ppgs", out, "--lenient", _scene(tmp_path, body)], capture_output=True, text=True)  # (not -q: the warnings are wanted)
    assert r.returncode == 0, r.stderr
    note = ("warning: subsurface plug-ins dropped (not supported)" if name == "subsurface" else
            "warning: participating media dropped (%d <medium> elements or references): this loader does not offer them" % (1 if name == "medium on a shape" else 3))
    assert note in r.stderr
    assert open(out, "rb").read() == flat_plain


# ------------------------------------------------------------------------------------------------ 4. the build stage
def test_ppg_set_scene_validation_and_tables_through_the_host_build_stage(tmp_path):
    """tests/media_build_check.hip: buildScene() without a context or a device, its host code under the address and undefined-behaviour
    sanitizers, as a child process"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found (set HIPCC)")
    exe = str(tmp_path / "media_build_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "media_build_check.hip")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout and "FAILED" not in run.stdout
    assert run.stdout.count("ok refused") == 21 and run.stdout.count("ok ") == 34
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
