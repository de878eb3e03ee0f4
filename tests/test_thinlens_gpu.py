"""The thin-lens camera on the GPU (include/ppg.h ppg_set_lens; ppg_kernels.h k_generate): the film of a defocused emitter equals a numpy
restatement of every sample's lens ray, an in-focus plane renders as through the pinhole, and sharding, the C++ driver, determinism and
the pinhole path are as for any other render."""
import os
import subprocess

import numpy as np
import pytest

from conftest import IMPROVED, ROOT
from test_rfilter_gpu import _rand
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu

W, H = 48, 40
ORIGIN = (0.1, -0.2, 0.0)
RECT = (-0.45, 0.35, -0.3, 0.25)  # x0, x1, y0, y1 of the emitter rectangle (world), in a plane z = const facing the camera
PROPS = dict(budgetType="spp", budget=16, sppPerPass=16, maxDepth=3, rrDepth=5, seed=19)


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def _rect_scene(z, lens):
    """a camera looking along +z from ORIGIN and one emitter rectangle (radiance 1, black BSDF) in the plane z: every sample's L is 1 or 0"""
    import ppg_host
    x0, x1, y0, y1 = RECT
    pos = np.array([(x0, y0, z), (x0, y1, z), (x1, y1, z), (x1, y0, z)], f32)  # normal -z: towards the camera
    idx = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
    cam = ppg_host.scenes.perspective_camera(ORIGIN, (ORIGIN[0], ORIGIN[1], 1.0), (0, 1, 0), 50.0, "x", 0.01, 100.0, W, H)
    return ppg_host.SceneDesc(pos, idx, np.zeros(2, np.uint32), np.zeros(2, np.int32), [dict(type=0, reflectance=(0.0, 0.0, 0.0))],
                              [dict(radiance=(1.0, 1.0, 1.0))], cam, lens=lens)


def _disk(u1, u2):
    """warp::squareToUniformDiskConcentric (warp.cpp:81-102)"""
    r1, r2 = 2.0 * u1 - 1.0, 2.0 * u2 - 1.0
    zero = (r1 == 0) & (r2 == 0)
    big = r1 * r1 > r2 * r2
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(big, r1, r2)
        phi = np.where(big, np.pi / 4 * (r2 / r1), np.pi / 2 - (r1 / r2) * (np.pi / 4))
    r, phi = np.where(zero, 0.0, r), np.where(zero, 0.0, phi)
    return r * np.cos(phi), r * np.sin(phi)


def _coverage(desc, z, seed, spp, lens=True):
    """per pixel: how many of samples 0 .. spp-1 hit the rectangle, and whether any of them lands within a relative 1e-4 of its edge"""
    cam = desc.camera
    s2c, c2w = np.asarray(cam["sample_to_camera"], np.float64), np.asarray(cam["camera_to_world"], np.float64)
    pix = np.arange(W * H, dtype=np.uint32)
    hits, grazing = np.zeros(W * H, np.int32), np.zeros(W * H, bool)
    x0, x1, y0, y1 = RECT
    for s in range(spp):
        u = [_rand(seed, pix, s, d).astype(np.float64) for d in range(4)]
        sx, sy = (pix % W) + u[0], (pix // W) + u[1]
        p = s2c @ np.stack([sx / W, sy / H, np.zeros_like(sx), np.ones_like(sx)])
        near = p[:3] / p[3]
        if lens:
            ax, ay = _disk(u[2], u[3])
            ap = np.stack([ax, ay, np.zeros_like(ax)]) * desc.lens["aperture_radius"]
            d = near * (desc.lens["focus_distance"] / near[2]) - ap
        else:
            ap, d = np.zeros_like(near), near
        d = d / np.linalg.norm(d, axis=0)
        o = c2w[:3, :3] @ ap + c2w[:3, 3:4]
        dw = c2w[:3, :3] @ d
        t = (z - o[2]) / dw[2]
        hx, hy = o[0] + t * dw[0], o[1] + t * dw[1]
        eps_x, eps_y = 1e-4 * (x1 - x0), 1e-4 * (y1 - y0)
        inside = (hx > x0) & (hx < x1) & (hy > y0) & (hy < y1)
        near_edge = ((np.abs(hx - x0) < eps_x) | (np.abs(hx - x1) < eps_x)) & (hy > y0 - eps_y) & (hy < y1 + eps_y)
        near_edge |= ((np.abs(hy - y0) < eps_y) | (np.abs(hy - y1) < eps_y)) & (hx > x0 - eps_x) & (hx < x1 + eps_x)
        hits += inside
        grazing |= near_edge
    return hits.reshape(H, W), grazing.reshape(H, W)


def _render(desc, **extra):
    e = hip(**dict(PROPS, **extra))
    e.set_scene(desc)
    e.render()
    film = e.read_film()
    e.close()
    return film


@pytest.mark.parametrize("env", ["", "PPG_FORCE_BVH"])
def test_defocused_film_is_the_numpy_lens_coverage(monkeypatch, env):
    """black emitter plane between camera and focal plane: the film of 16 samples is (samples that hit) / 16 in every pixel"""
    if env:
        monkeypatch.setenv(env, "1")
    z = 2.0
    desc = _rect_scene(z, dict(aperture_radius=0.06, focus_distance=5.0))
    film = _render(desc)
    hits, grazing = _coverage(desc, z, PROPS["seed"], 16)
    want = (hits.astype(f32) / f32(16))[..., None] * np.ones(3, f32)
    ok = ~grazing
    assert grazing.sum() <= 0.02 * W * H
    assert np.array_equal(film[ok], want[ok]), np.argwhere((film != want).any(-1) & ok)[:10]
    partial = (hits > 0) & (hits < 16)
    assert partial.sum() > 0.05 * W * H  # the edges are blurred over several pixels
    assert (hits == 16).any() and (hits == 0).any()


def test_in_focus_plane_renders_as_through_the_pinhole():
    z = 3.0
    pin = _rect_scene(z, None)
    focused = _rect_scene(z, dict(aperture_radius=0.08, focus_distance=z - ORIGIN[2]))
    f_pin, f_lens = _render(pin), _render(focused)
    _, grazing = _coverage(pin, z, PROPS["seed"], 16, lens=False)
    _, grazing_lens = _coverage(focused, z, PROPS["seed"], 16)
    ok = ~(grazing | grazing_lens)
    assert ok.sum() > 0.9 * W * H
    assert np.array_equal(f_lens[ok], f_pin[ok])
    assert (f_pin > 0).any() and (f_pin == 0).any()
    defocused = _render(_rect_scene(z, dict(aperture_radius=0.08, focus_distance=1.0)))
    assert ((defocused != f_pin).any(-1) & ok).sum() > 0.05 * W * H


def test_lens_scene_renders_the_same_when_sharded(tmp_path):
    """two ranks on one GPU (test_two_ranks_one_gpu.py's workers: tiles, optimiser rounds, final groups) against one unsharded render"""
    import ppg_host
    from test_two_ranks_one_gpu import _launch, _unsharded
    from conftest import CBOX_PROPS
    desc = ppg_host.cbox_scene(96, 96)
    desc.lens = dict(aperture_radius=12.0, focus_distance=900.0)
    path = str(tmp_path / "cbox-lens.ppgs")
    ppg_host.save_scene(desc, path)
    case = dict(scene=path, res=[96, 96], tile=16, props=dict(CBOX_PROPS, budget=31.0, seed=6, **IMPROVED))
    img, tree, gpt = _unsharded(case)
    assert gpt.engine._lens is not None
    pin_img, _, _ = _unsharded(dict(case, scene="cbox"))
    assert not np.array_equal(img, pin_img)
    for r in _launch(tmp_path, case):
        assert np.array_equal(r["film"], img)
        assert np.array_equal(r["children"], tree["children"]) and np.array_equal(r["dch"], tree["sampling"]["node_children"])
        assert np.array_equal(r["dsum"], tree["sampling"]["node_sums"]) and np.array_equal(r["theta"], tree["theta"])


def test_cpp_driver_equals_python_on_a_lens_scene(tmp_path):
    import ppg_host
    from test_cpp_host import read_pfm
    exe = os.path.join(ROOT, "practical-path-guiding_amd", "bin", "ppg_render")
    desc = ppg_host.cbox_scene(64, 48)
    desc.lens = dict(aperture_radius=20.0, focus_distance=700.0)
    path = str(tmp_path / "cbox-lens.ppgs")
    ppg_host.save_scene(desc, path)
    props = dict(budgetType="spp", budget=28, maxDepth=10, rrDepth=10, strictNormals=1, seed=4, **{k: v for k, v in IMPROVED.items() if k != "sppPerPass"})
    out = str(tmp_path / "out.pfm")
    args = [exe, "-q", "-o", out] + sum([["-D", "%s=%s" % kv] for kv in props.items()], [])
    r = subprocess.run(args + [path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.load_scene_file(path))
    assert np.array_equal(read_pfm(out), img) and img.mean() > 0


def test_lens_render_is_deterministic():
    import ppg_host
    desc = ppg_host.cbox_scene(64, 48)
    desc.lens = dict(aperture_radius=15.0, focus_distance=600.0)
    props = dict(budgetType="spp", budget=31, sppPerPass=1, maxDepth=-1, rrDepth=5, nee="always", seed=23, **{k: v for k, v in IMPROVED.items() if k != "sppPerPass"})
    out = []
    for _ in range(2):
        gpt = ppg_host.GuidedPathTracer(engine=hip(**props))
        img = gpt.render(desc)
        out.append((img, gpt.engine.read_sdtree(), gpt.iterations))
    assert np.array_equal(out[0][0], out[1][0]) and np.isfinite(out[0][0]).all() and out[0][0].mean() > 0
    _tree_equal(out[0][1], out[1][1])
    for it in out[0][2]:
        st = it.get("tree")
        if st is not None:
            vals = [v for v in (st.values() if isinstance(st, dict) else vars(st).values()) if isinstance(v, (int, float))]
            assert all(np.isfinite(v) for v in vals)


def test_set_lens_refuses_bad_values():
    import ppg_host
    from ppg_host.bindings import PPGError
    e = hip(budgetType="spp", budget=4)
    e.set_scene(ppg_host.cbox_scene(16, 16))
    for bad in (dict(aperture_radius=0.0, focus_distance=1.0), dict(aperture_radius=-0.1, focus_distance=1.0),
                dict(aperture_radius=float("nan"), focus_distance=1.0), dict(aperture_radius=float("inf"), focus_distance=1.0)):
        with pytest.raises(PPGError, match="aperture_radius must be finite and > 0") as ex:
            e.set_lens(bad)
        assert ex.value.code == -1
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(PPGError, match="focus_distance must be finite and > 0") as ex:
            e.set_lens(dict(aperture_radius=0.1, focus_distance=bad))
        assert ex.value.code == -1
    e.set_lens(dict(aperture_radius=0.1, focus_distance=1.0))
    e.set_lens(None)


def test_pinhole_after_a_lens_render_is_the_pinhole():
    import ppg_host
    props = dict(budgetType="spp", budget=12, maxDepth=10, rrDepth=10, strictNormals=1, seed=8)
    desc = ppg_host.cbox_scene(48, 40)
    fresh = hip(**props)
    fresh.set_scene(desc)
    fresh.render()
    want = fresh.read_film()
    e = hip(**props)
    e.set_scene(desc)
    e.set_lens(dict(aperture_radius=25.0, focus_distance=500.0))
    e.render()
    lens_film = e.read_film()
    e.set_lens(None)
    e.render()
    assert np.array_equal(e.read_film(), want) and not np.array_equal(lens_film, want)
    # and through a scene description without a lens after one with a lens
    g = hip(**props)
    lensed = ppg_host.cbox_scene(48, 40)
    lensed.lens = dict(aperture_radius=25.0, focus_distance=500.0)
    g.set_scene(lensed)
    g.render()
    assert np.array_equal(g.read_film(), lens_film)
    g.set_scene(desc)
    g.render()
    assert np.array_equal(g.read_film(), want)
