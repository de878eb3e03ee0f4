"""ppg_set_scene builds a scene on the host first and touches the context only once the scene is accepted (include/ppg.h: PPG_ERR_INVALID
leaves the previous scene set).  A refused scene therefore leaves the previous one renderable — bit for bit, without another set_scene —
and ppg_set_lens afterwards still builds the scene box from what the set scene was built with.

Every refused scene here is one whose defect ppg_set_scene finds late — after the microfacet table, the texture coordinates, the texels or
the whole geometry of an accepted scene would be on the device — and each has fewer materials and textures than the good scene and more
triangles, so every buffer involved would have shrunk in content and grown in size."""
import numpy as np
import pytest

from conftest import CBOX_PROPS

f32 = np.float32
pytestmark = pytest.mark.gpu
PROPS = dict(CBOX_PROPS, budget=4, sppPerPass=1, seed=11)  # 4 passes of 1 spp


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def _texels(n, seed):
    return np.random.default_rng(seed).uniform(0.1, 0.9, (n, n, 3)).astype(f32)


def _quads(quads, materials, emitters, textures, **more):
    """quads: (four corners, material, emitter); every quad carries the texture coordinates of the unit square"""
    from ppg_host.scenes import SceneDesc, perspective_camera
    pos, uv, idx, tmat, tem = [], [], [], [], []
    for verts, mat, em in quads:
        base = len(pos)
        pos.extend(verts)
        uv.extend([(0, 0), (1, 0), (1, 1), (0, 1)])
        idx.extend([(base, base + 1, base + 2), (base, base + 2, base + 3)])
        tmat.extend([mat] * 2)
        tem.extend([em] * 2)
    cam = perspective_camera((0.5, 1.0, -2.5), (0.5, 0.4, 0.5), (0, 1, 0), 40.0, "smaller", 0.1, 100.0, 32, 32)
    return SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array(tmat, np.uint32), np.array(tem, np.int32), materials, emitters, cam,
                     texcoords=np.array(uv, f32), textures=textures, **more)


LIGHT = ([(0.25, 1.5, 0.25), (0.75, 1.5, 0.25), (0.75, 1.5, 0.75), (0.25, 1.5, 0.75)], 1, 0)


def scene_a(**more):
    """a textured floor and an anisotropic rough-conductor wall (a general microfacet entry with an alphaV bitmap) under an area light:
    3 materials, two 4x4 textures, 6 triangles"""
    floor = ([(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0)], 0, -1)
    wall = ([(0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 1)], 2, -1)
    materials = [dict(type=0, reflectance=(0.8, 0.8, 0.8), texture=0), dict(type=0, reflectance=(0.5, 0.5, 0.5)),
                 dict(type="roughconductor", eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), alpha=0.1, alpha_v=0.3, alpha_v_texture=1)]
    return _quads([floor, wall, LIGHT], materials, [dict(radiance=(20.0, 18.0, 15.0))], [dict(rgb=_texels(4, 1)), dict(rgb=0.5 * _texels(4, 2))], **more)


def scene_b(materials, textures=None, **more):
    """the same room with a floor of 4 x 4 quads: 2 materials, at most one 2x2 texture, 34 triangles"""
    quads = []
    for i in range(4):
        for j in range(4):
            x0, x1, z0, z1 = i / 4, (i + 1) / 4, j / 4, (j + 1) / 4
            quads.append(([(x0, 0, z0), (x0, 0, z1), (x1, 0, z1), (x1, 0, z0)], 0, -1))
    textures = [dict(rgb=_texels(2, 3))] if textures is None else textures
    return _quads(quads + [LIGHT], materials, [dict(radiance=(1.0, 2.0, 3.0))], textures, **more)


PLAIN = [dict(type=0, reflectance=(0.2, 0.3, 0.4), texture=0), dict(type=0, reflectance=(0.5, 0.5, 0.5))]


def _bad_coating():  # refused by the coatings' checks: the microfacet table of material 0 would be on the device by then
    return scene_b([dict(type="roughconductor", eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), alpha=0.2, alpha_v=0.4, texture=0),
                    dict(type=0, reflectance=(0.5, 0.5, 0.5), coating=dict(kind="coating", eta=1.0, thickness=1.0))])


def _blend_child_out_of_range():
    from ppg_host.bindings import Blend
    desc = scene_b([dict(type=0, reflectance=(0.0, 0.0, 0.0)), dict(type=0, reflectance=(0.5, 0.5, 0.5))], textures=[])
    b = Blend()
    b.kind, b.n, b.child[0], b.child[1], b.weight[0] = 1, 2, 1, 2, 0.5
    desc.blends = [b, Blend()]
    return desc


REFUSED = [  # (name, scene, what the message says)
    ("bad-coating", _bad_coating, "coating"),
    ("blend-child-out-of-range", _blend_child_out_of_range, "index out of range"),
    ("texture-of-width-0", lambda: scene_b(PLAIN, textures=[dict(rgb=np.zeros((2, 0, 3), f32))]), "texture: needs pixels"),
    ("environment-and-envmap", lambda: scene_b(PLAIN, environment=(1.0, 1.0, 1.0), envmap=dict(rgb=np.ones((2, 4, 3), f32))), "one environment emitter"),
    ("black-envmap", lambda: scene_b(PLAIN, envmap=dict(rgb=np.zeros((2, 4, 3), f32))), "completely black"),
]


@pytest.fixture(scope="module")
def engine_and_film():
    e = hip(**PROPS)
    e.set_scene(scene_a())
    e.render()
    film = e.read_film()
    assert np.isfinite(film).all() and film.mean() > 0.01
    yield e, film
    e.close()


@pytest.mark.parametrize("k", range(len(REFUSED)), ids=[r[0] for r in REFUSED])
def test_a_refused_scene_leaves_the_previous_one_renderable(engine_and_film, k):
    from ppg_host.bindings import PPGError
    engine, film = engine_and_film
    name, build, says = REFUSED[k]
    with pytest.raises(PPGError) as err:
        engine.set_scene(build())
    assert err.value.code == -1 and says in str(err.value), str(err.value)  # PPG_ERR_INVALID
    engine.render()  # no set_scene in between: the scene is still A
    again = engine.read_film()
    assert np.array_equal(again, film), "max abs difference %g" % np.abs(again - film).max()


def test_set_lens_after_a_refused_scene_keeps_the_set_scenes_box():
    """The scene box holds the positions of the point emitters (Scene::getAABB); ppg_set_lens builds it again.  After a refused scene with
    another list of emitters the box must still be the one of the scene that is set: the first iteration's tree box equals a fresh context's."""
    from ppg_host.bindings import PPGError
    lens = dict(aperture_radius=0.05, focus_distance=3.0)
    point_a = [dict(type="point", intensity=(5.0, 5.0, 5.0), position=(0.5, 4.0, 0.5))]
    point_b = [dict(type="point", intensity=(5.0, 5.0, 5.0), position=(9.0, 0.5, -7.0)), dict(type="point", intensity=(1.0, 1.0, 1.0), position=(-6.0, 0.5, 0.5))]

    def tree_box(e):
        e.set_lens(lens)
        e.begin_render()
        info = e.sdtree_info()
        e.end_render()
        return np.array(list(info.aabb_min) + list(info.aabb_max), f32)

    fresh = hip(**PROPS)
    fresh.set_scene(scene_a(delta_emitters=point_a))
    expected = tree_box(fresh)
    fresh.close()
    assert expected[4] > 3.9  # the emitter of A is inside

    e = hip(**PROPS)
    e.set_scene(scene_a(delta_emitters=point_a))
    with pytest.raises(PPGError) as err:
        e.set_scene(scene_b(PLAIN, envmap=dict(rgb=np.zeros((2, 4, 3), f32)), delta_emitters=point_b))
    assert err.value.code == -1
    got = tree_box(e)
    e.close()
    assert np.array_equal(got, expected), (got, expected)
