"""Film reconstruction filters on the GPU (include/ppg.h ppg_set_rfilter; ppg_kernels.h k_film_filter / k_film_resolve): the filtered film
equals a numpy splat of the same samples, summed in the documented order; learning, determinism and the default box path are untouched."""
import ctypes as C

import numpy as np
import pytest

from conftest import IMPROVED

f32 = np.float32
pytestmark = pytest.mark.gpu


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def _hash(x):
    x = np.asarray(x, np.uint32)
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _rand(seed, pixel, sample, dim):
    """include/ppg_rng.h ppg_path_key + ppg_rand"""
    with np.errstate(over="ignore"):
        k = _hash(np.uint32(seed & 0xffffffff) ^ np.uint32(0x9e3779b9))
        k = _hash(k ^ np.uint32(seed >> 32))
        k = _hash(k + pixel.astype(np.uint32) * np.uint32(0x9e3779b1))
        k = _hash(k ^ (np.uint32(sample) * np.uint32(0x85ebca77) + np.uint32(0xc2b2ae3d)))
        r = _hash(k ^ _hash(np.uint32(dim) * np.uint32(0x9e3779b1) + np.uint32(0x7f4a7c15)))
    return ((r >> np.uint32(9)) | np.uint32(0x3f800000)).view(f32) - f32(1)


def np_splat(L, rf, seed, sample=0):
    """the film of ONE sample per pixel (index `sample`), radiance L[h, w, 3], splatted with filter `rf` (ImageBlock::put) and summed per
    target pixel over its taps dy = -B..B, dx = -B..B (include/ppg.h), then normalised as ppg_read_film does"""
    import ppg_host.bindings as b
    table, r, B = b.rfilter_table(rf)
    r, scale = f32(r), f32(31) / f32(r)
    H, W = L.shape[:2]
    pix = np.arange(H * W, dtype=np.uint32)
    posx = ((pix % W).astype(f32) + _rand(seed, pix, sample, 0)) - f32(0.5)
    posy = ((pix // W).astype(f32) + _rand(seed, pix, sample, 1)) - f32(0.5)
    posx, posy = posx.reshape(H, W), posy.reshape(H, W)
    ty, tx = np.mgrid[0:H, 0:W]
    S = np.zeros((H, W, 4), f32)
    for dy in range(-B, B + 1):
        for dx in range(-B, B + 1):
            sy, sx = ty - dy, tx - dx
            ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
            syc, sxc = np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)
            px, py = posx[syc, sxc], posy[syc, sxc]
            ylo = np.maximum(np.ceil(py - r).astype(np.int64), 0); yhi = np.minimum(np.floor(py + r).astype(np.int64), H - 1)
            xlo = np.maximum(np.ceil(px - r).astype(np.int64), 0); xhi = np.minimum(np.floor(px + r).astype(np.int64), W - 1)
            ok &= (ty >= ylo) & (ty <= yhi) & (tx >= xlo) & (tx <= xhi)
            wy = table[np.minimum(np.abs((ty.astype(f32) - py) * scale).astype(np.int64), 31)]
            wx = table[np.minimum(np.abs((tx.astype(f32) - px) * scale).astype(np.int64), 31)]
            w = wx * wy
            c = np.concatenate([w[..., None] * L[syc, sxc], w[..., None]], axis=2)
            S = S + np.where(ok[..., None], c, f32(0))
    iw = np.where(S[..., 3] != 0, f32(1) / np.where(S[..., 3] != 0, S[..., 3], f32(1)), f32(0)).astype(f32)
    return S[..., :3] * iw[..., None]


FILTERS = [{"type": "gaussian"}, {"type": "tent"}, {"type": "box", "radius": 1.5}, {"type": "mitchell"}, {"type": "catmullrom"},
           {"type": "lanczos"}, {"type": "lanczos", "lobes": 2}, {"type": "gaussian", "stddev": 0.3}]


def _scene(name):
    import ppg_host
    return ppg_host.cbox_scene(67, 41) if name == "cbox" else ppg_host.room_scene(67, 41, n_boxes=40, tess=1)


@pytest.mark.parametrize("scene", ["cbox", "room"])
def test_filtered_film_is_the_exact_splat(scene):
    """one final pass of one sample per pixel: box gives each pixel's L; every filter's film is the numpy splat of those L"""
    props = dict(budgetType="spp", budget=1, sppPerPass=1, maxDepth=6, rrDepth=5, seed=7)
    desc = _scene(scene)
    e = hip(**props)
    e.set_scene(desc)
    e.render()
    L = e.read_film().astype(f32)
    assert L.mean() > 0
    for rf in FILTERS:
        desc.rfilter = rf
        g = hip(**props)
        g.set_scene(desc)
        g.render()
        got, want = g.read_film(), np_splat(L, rf, 7)
        assert np.allclose(got, want, rtol=2e-6, atol=0), (rf, np.abs(got - want).max())
        g.close()


def test_training_pass_is_the_exact_splat():
    """the same through a training iteration (one ppg_render_passes call, not the final groups)"""
    props = dict(budgetType="spp", budget=64, sppPerPass=1, maxDepth=6, rrDepth=5, seed=3)
    desc = _scene("cbox")
    films = {}
    for rf in (None, {"type": "gaussian"}, {"type": "lanczos"}):
        desc.rfilter = rf
        e = hip(**props)
        e.set_scene(desc)
        e.begin_render()
        e.begin_iteration(0)
        e.render_passes(1)
        films[str(rf)] = e.read_film()
        e.close()
    L = films["None"].astype(f32)
    for rf in ({"type": "gaussian"}, {"type": "lanczos"}):
        assert np.allclose(films[str(rf)], np_splat(L, rf, 3), rtol=2e-6, atol=0), rf


def _improved_render(rf, monkeypatch=None, env=()):
    import ppg_host
    for k, v in env:
        monkeypatch.setenv(k, v)
    props = dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=11)
    desc = ppg_host.cbox_scene(67, 41)
    desc.rfilter = rf
    e = hip(**props)
    e.set_scene(desc)
    e.render()
    out = e.read_film(), e.read_sdtree()
    e.close()
    for k, _ in env:
        monkeypatch.delenv(k)
    return out


def _tree_equal(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _tree_equal(a[k], b[k])
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b)
    else:
        assert a == b


def test_learning_is_untouched_by_the_filter():
    fb, tb = _improved_render(None)
    fg, tg = _improved_render({"type": "gaussian"})
    _tree_equal(tb, tg)  # SD-tree and the learned sampling fractions (its "theta")
    assert "theta" in tb and np.isfinite(fb).all() and not np.array_equal(fb, fg)


@pytest.mark.parametrize("env", [(("PPG_BATCH_PATHS", "20000"),), (("PPG_BLOCKS", "512"),), (("PPG_NO_OVERLAP", "1"),),
                                 (("PPG_FINAL_HALVES", "1"), ("PPG_SPLIT_DEPTH", "4"))], ids=lambda e: "+".join(k for k, _ in e))
def test_filtered_film_is_deterministic(monkeypatch, env):
    ref = _improved_render({"type": "gaussian"})[0]
    assert np.array_equal(ref, _improved_render({"type": "gaussian"})[0])
    assert np.array_equal(ref, _improved_render({"type": "gaussian"}, monkeypatch, env)[0])


def test_default_box_set_explicitly_is_the_unfiltered_path():
    import ppg_host
    props = dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, seed=5)
    desc = ppg_host.cbox_scene(67, 41)
    a = hip(**props)
    a.set_scene(desc)
    a.render()
    b = hip(**props)
    b.set_scene(desc)
    b.set_rfilter({"type": "box", "radius": 0.5})
    b.render()
    film = a.read_film()
    assert np.isfinite(film).all() and np.array_equal(film, b.read_film())


def test_constant_radiance_is_kept():
    """a uniform environment and nothing in view: every filter's film is the radiance"""
    import ppg_host
    desc = ppg_host.cbox_scene(45, 37)
    # one small triangle behind the camera stands in for "no geometry"
    c2w = np.asarray(desc.camera["camera_to_world"], f32)
    o, fwd = c2w[:3, 3], c2w[:3, 2]
    back = o - 50 * fwd
    desc.positions = np.array([back, back + [1, 0, 0], back + [0, 1, 0]], f32)
    desc.normals = None
    desc.indices = np.array([[0, 1, 2]], np.uint32)
    desc.tri_material = np.zeros(1, np.uint32)
    desc.tri_emitter = np.full(1, -1, np.int32)
    desc.emitters = []
    desc.environment = (0.25, 0.5, 0.75)
    for rf in ({"type": "gaussian"}, {"type": "tent"}, {"type": "box", "radius": 1.5}):
        desc.rfilter = rf
        e = hip(budgetType="spp", budget=8, maxDepth=4, seed=2)
        e.set_scene(desc)
        e.render()
        img = e.read_film()
        assert np.allclose(img, np.array([0.25, 0.5, 0.75], f32), rtol=0, atol=1e-5), (rf, np.abs(img - [0.25, 0.5, 0.75]).max())
        e.close()


def test_sharding_a_filtered_render_is_refused():
    import ppg_host
    from ppg_host.bindings import PPGError
    desc = ppg_host.cbox_scene(16, 16)
    e = hip(budgetType="spp", budget=4)
    e.set_scene(desc)
    e.set_rfilter({"type": "gaussian"})
    with pytest.raises(PPGError, match="sharded filtered renders are not supported yet") as ex:
        e.set_shard(0, 2, 32)
    assert ex.value.code == -1
    f = hip(budgetType="spp", budget=4)
    f.set_scene(desc)
    f.set_shard(1, 2, 32)
    with pytest.raises(PPGError, match="sharded filtered renders are not supported yet") as ex:
        f.set_rfilter({"type": "gaussian"})
    assert ex.value.code == -1
    f.set_rfilter(None)  # the default box is fine
