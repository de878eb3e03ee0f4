"""Engine.set_scene sends every side list of the C-ABI with the scene, and an empty list clears what the context held: a plain scene after
a scene that carried them all renders the picture a fresh context renders.  The C++ hosts send them with SceneData::apply: a refused
scene names the call that refused it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import CBOX_PROPS, PKG

pytestmark = pytest.mark.gpu

PROPS = dict(CBOX_PROPS, budget=48, seed=11, nee="always")  # 12 passes of 4 spp


def loaded_cbox(w=16, h=16):
    """The Cornell box on its own five materials, with as many side lists as one scene may combine: a masked mixturebsdf (blends, and a
    bitmap on the opacity: material textures), an anisotropic roughconductor (microfacet), a coated light (coatings), a point emitter, a
    disk, a gaussian film filter and a thin lens.  Five materials, so that each per-material list has the length the plain box expects."""
    import ppg_host
    desc = ppg_host.cbox_scene(w, h)
    box, white, red, green, light = (dict(m) for m in desc.materials)
    desc.materials = [
        dict(type=0, opacity=(0.5, 0.5, 0.5), opacity_texture=0, blend=dict(kind="mixturebsdf", children=[2, 3], weights=(0.6, 0.4))),
        dict(type="roughconductor", alpha=0.2, alpha_v=0.05, eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), reflectance=(1.0, 1.0, 1.0)),
        red, green, dict(light, coating=dict(kind="coating", eta=1.5, thickness=1.0, sigma_a=(0.1, 0.2, 0.3)))]
    assert len(desc.materials) == 5
    pos = np.asarray(desc.positions, np.float32)
    desc.texcoords = np.ascontiguousarray(pos[:, [0, 2]] / np.float32(560.0))
    desc.textures = [dict(rgb=np.asarray([[(0.2, 0.2, 0.2), (0.8, 0.8, 0.8)]], np.float32), nearest=True)]
    desc.delta_emitters = [dict(type="point", intensity=(4e4, 3e4, 2e4), position=(278.0, 400.0, 280.0))]
    desc.shapes = [dict(type="disk", to_world=[60, 0, 0, 420, 0, 0, 60, 1.0, 0, -60, 0, 120], material=2)]
    desc.rfilter = dict(type="gaussian", stddev=0.5)
    desc.lens = dict(aperture_radius=8.0, focus_distance=1000.0)
    return desc


def _film(engine, desc):
    engine.set_scene(desc)
    engine.render()
    return engine.read_film()


def test_a_plain_scene_after_a_scene_with_every_side_list_renders_as_on_a_fresh_context():
    import ppg_host
    fresh = ppg_host.Engine.hip(**PROPS)
    want = _film(fresh, ppg_host.cbox_scene(16, 16))
    fresh.close()
    used = ppg_host.Engine.hip(**PROPS)
    first = _film(used, loaded_cbox())
    got = _film(used, ppg_host.cbox_scene(16, 16))
    used.close()
    assert np.isfinite(first).all() and first.mean() > 0.01 and not np.array_equal(first, want)
    assert np.isfinite(want).all() and want.mean() > 0.01
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case, call, says", [("delta", "ppg_set_delta_emitters", "delta emitter 0: negative intensity"),
                                              ("shape", "ppg_set_scene", "its transformation is singular")])
def test_the_cpp_hosts_name_the_setter_that_refused_the_scene(tmp_path, case, call, says):
    """GuidedPathTracerHIP::render throws "<call>: " + ppg_last_error, which the driver prints behind "error: "; PluginCore::render hands
    back ppg_last_error alone.  One scene refused by a side list's own setter, one by ppg_set_scene behind the lists."""
    import ppg_host
    desc = ppg_host.cbox_scene(16, 16)
    if case == "delta":
        desc.delta_emitters = [dict(type="point", intensity=(-1.0, 1.0, 1.0), position=(278.0, 400.0, 280.0))]
    else:
        desc.shapes = [dict(type="disk", to_world=[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0], material=2)]
    path = str(tmp_path / "refused.ppgs")
    ppg_host.save_scene(desc, path)
    exe = os.path.join(PKG, "bin", "ppg_render")
    defs = sum([["-D", "%s=%s" % kv] for kv in dict(CBOX_PROPS, budget=4).items()], [])
    r = subprocess.run([exe, "-q", "-o", str(tmp_path / "a.pfm")] + defs + [path], capture_output=True, text=True, timeout=120)
    errors = [line for line in r.stderr.splitlines() if line.startswith("error: ")]
    assert r.returncode == 3 and len(errors) == 1 and errors[0].startswith("error: %s: " % call) and says in errors[0], (r.returncode, r.stderr)
    r = subprocess.run([exe, "-q", "--plugin-core", "-o", str(tmp_path / "b.pfm")] + defs + [path], capture_output=True, text=True, timeout=120)
    errors = [line for line in r.stderr.splitlines() if line.startswith("error: ")]
    assert r.returncode == 3 and len(errors) == 1 and says in errors[0] and call not in errors[0], (r.returncode, r.stderr)
    assert not (tmp_path / "a.pfm").exists() and not (tmp_path / "b.pfm").exists()
