/*
 * normalmap_build_check.hip — buildScene() (csrc/ppg_scene_build.h), the pure stage of ppg_set_scene, on the normalmap adapter
 * (PPG_MAT_NORMALMAP) and the null BSDF (PPG_BSDF_NULL), without a context and without a device: the scenes it accepts — and which kernel
 * family they ask for —, and every refusal with its exact message.  A refused build returns before anything is committed: the program
 * also checks that the inputs of a refused scene build again, unchanged, once the defect is taken out.  Built with the host sanitizers
 * and run by tests/test_normalmap.py.
 */
#include <cstdio>
#include <functional>

#include "../practical-path-guiding_amd/csrc/ppg_scene_build.h"

namespace {

enum { M_DIFFUSE, M_SUBJECT, M_OTHER, N_MATERIALS };  // the quad's own material, the material under test (on no triangle unless a case puts it there), a plain diffuse

struct Fixture {
    std::vector<float> positions{0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0}, texels{0.5f, 0.5f, 1.0f, 0.6f, 0.5f, 0.9f, 0.5f, 0.6f, 0.9f, 0.4f, 0.5f, 0.9f};
    std::vector<uint32_t> indices{0, 1, 2, 0, 2, 3}, triMaterial{M_DIFFUSE, M_DIFFUSE};
    std::vector<int32_t> triEmitter{0, -1};
    std::vector<ppg_material> materials;
    std::vector<ppg_emitter> emitters{ppg_emitter{{5.0f, 5.0f, 5.0f}, 0.0f}};
    std::vector<ppg_sphere> spheres;
    std::vector<ppg_texture> textures;
    ppg_scene scene{};
    std::vector<ppg_material_textures> materialTextures;
    std::vector<ppg_microfacet> microfacet;
    std::vector<ppg_coating> coatings;
    std::vector<ppg_blend> blends;
    std::vector<ppg_delta_emitter> deltaEmitters;
    std::vector<ppg_shape> shapes;

    Fixture() {
        materials.resize(N_MATERIALS);
        for (auto &m : materials) {
            m = ppg_material{};
            m.type = PPG_BSDF_DIFFUSE;
            for (int c = 0; c < 3; ++c) { m.reflectance[c] = 0.5f; m.specular[c] = 1.0f; m.eta[c] = 1.5f; m.k[c] = 1.0f; m.opacity[c] = 0.5f; }
            m.alpha = 0.1f;
        }
        ppg_texture t{};
        t.width = t.height = 2;
        t.uv_scale[0] = t.uv_scale[1] = 1.0f;
        textures = {t};
        ppg_scene &s = scene;
        s.n_vertices = 4; s.n_triangles = 2; s.n_materials = N_MATERIALS; s.n_emitters = 1; s.n_textures = 1;
        const float c2w[16] = {1, 0, 0, 0.5f, 0, 1, 0, 0.5f, 0, 0, -1, 3.0f, 0, 0, 0, 1};
        const float s2c[16] = {1, 0, 0, -0.5f, 0, 1, 0, -0.5f, 0, 0, 1, 0, 0, 0, 1, 0};
        memcpy(s.camera.camera_to_world, c2w, sizeof c2w); memcpy(s.camera.sample_to_camera, s2c, sizeof s2c);
        s.camera.near_clip = 0.1f; s.camera.far_clip = 100.0f; s.camera.width = 8; s.camera.height = 8;
    }
    void null(uint32_t i = M_SUBJECT) { materials[i].type = PPG_BSDF_NULL; }
    void normalMapped(uint32_t i = M_SUBJECT) { materials[i].flags |= PPG_MAT_NORMALMAP; materials[i].texture = 1u << 16; }
    void onTheQuad(uint32_t i = M_SUBJECT) { triMaterial[0] = triMaterial[1] = i; }
    void sphere() {
        ppg_sphere sp{};
        sp.center[0] = 0.5f; sp.center[1] = 0.5f; sp.center[2] = 1.0f; sp.radius = 0.25f;
        sp.to_world[0] = sp.to_world[4] = sp.to_world[8] = 1.0f;
        sp.material = M_SUBJECT; sp.emitter = -1;
        spheres = {sp};
    }
    void disk() {
        ppg_shape d{};
        const float toWorld[12] = {0.25f, 0, 0, 0.5f, 0, 0.25f, 0, 0.5f, 0, 0, 0.25f, 1.0f};
        d.type = PPG_SHAPE_DISK; memcpy(d.to_world, toWorld, sizeof toWorld); d.material = M_SUBJECT; d.emitter = -1;
        shapes = {d};
    }
    SceneInputs inputs() {
        ppg_scene &s = scene;
        s.positions = positions.data(); s.indices = indices.data(); s.tri_material = triMaterial.data(); s.tri_emitter = triEmitter.data();
        s.materials = materials.data(); s.emitters = emitters.data(); s.textures = textures.data();
        s.n_spheres = (uint32_t)spheres.size(); s.spheres = spheres.empty() ? nullptr : spheres.data();
        textures[0].rgb = texels.data();
        return SceneInputs{&scene, materialTextures, microfacet, coatings, blends, deltaEmitters, shapes, nullptr, 2e-6f, 4, false};
    }
};

int failures = 0;

void accepted(const char *name, const std::function<void(Fixture &)> &prepare, int lobes, int hasNull) {
    Fixture f;
    prepare(f);
    HostScene H;
    std::string err;
    const int rc = buildScene(f.inputs(), H, err);
    if (rc == PPG_OK && H.scene.lobes == lobes && H.scene.has_null == hasNull && (H.fullMaterials || !lobes)) { printf("ok accepted %s\n", name); return; }
    printf("FAILED accepted %s: code %d, message \"%s\", lobes %d (expected %d), has_null %d (expected %d), fullMaterials %d\n", name, rc, err.c_str(), H.scene.lobes, lobes,
           H.scene.has_null, hasNull, (int)H.fullMaterials);
    ++failures;
}

void refused(const char *name, const std::function<void(Fixture &)> &spoil, const std::string &message) {
    Fixture f;
    spoil(f);
    HostScene H;
    std::string err;
    const int rc = buildScene(f.inputs(), H, err);
    if (rc == PPG_ERR_INVALID && err == message) { printf("ok refused %s\n", name); return; }
    printf("FAILED refused %s: code %d, message \"%s\", expected \"%s\"\n", name, rc, err.c_str(), message.c_str());
    ++failures;
}

}  // namespace

int main() {
    accepted("plain", [](Fixture &) {}, 0, 0);
    accepted("normal-mapped, unused", [](Fixture &f) { f.normalMapped(); }, 2, 0);
    accepted("normal-mapped, on the quad", [](Fixture &f) { f.normalMapped(); f.onTheQuad(); }, 2, 0);
    accepted("normal-mapped, masked and two-sided", [](Fixture &f) { f.normalMapped(); f.materials[M_SUBJECT].flags |= PPG_MAT_MASK | PPG_MAT_TWOSIDED; f.onTheQuad(); }, 2, 1);
    accepted("normal-mapped with a reflectance bitmap", [](Fixture &f) { f.normalMapped(); f.materials[M_SUBJECT].texture |= 1u; f.onTheQuad(); }, 2, 0);
    accepted("bump-mapped (no flag): the family it had", [](Fixture &f) { f.materials[M_SUBJECT].texture = 1u << 16; f.onTheQuad(); }, 0, 0);
    accepted("null, unused", [](Fixture &f) { f.null(); }, 2, 1);
    accepted("null, on the quad, one triangle an emitter", [](Fixture &f) { f.null(); f.onTheQuad(); }, 2, 1);
    accepted("null beside a roughdiffuse", [](Fixture &f) { f.null(); f.materials[M_OTHER].type = PPG_BSDF_ROUGHDIFFUSE; }, 3, 1);
    accepted("a normal-mapped blend record", [](Fixture &f) {
        f.normalMapped();
        f.blends.assign(N_MATERIALS, ppg_blend{});
        ppg_blend &b = f.blends[M_SUBJECT];
        b.kind = 1; b.n = 2; b.child[0] = M_DIFFUSE; b.child[1] = M_OTHER; b.weight[0] = 0.5f;
        f.onTheQuad();
    }, 2, 0);

    const std::string who = "material 1: ";
    refused("the flag without a normal map", [](Fixture &f) { f.materials[M_SUBJECT].flags |= PPG_MAT_NORMALMAP; },
            who + "PPG_MAT_NORMALMAP without a normal map: bits 16..31 of `texture` are 0");
    refused("the flag with a reflectance bitmap only", [](Fixture &f) { f.materials[M_SUBJECT].flags |= PPG_MAT_NORMALMAP; f.materials[M_SUBJECT].texture = 1u; },
            who + "PPG_MAT_NORMALMAP without a normal map: bits 16..31 of `texture` are 0");
    refused("a normal map out of range", [](Fixture &f) { f.normalMapped(); f.materials[M_SUBJECT].texture = 2u << 16; }, "material.texture: index out of range");
    refused("normal-mapped on a sphere", [](Fixture &f) { f.normalMapped(); f.sphere(); }, "sphere: textured BSDFs are only supported on triangle meshes (not on spheres, disks or cylinders)");
    refused("normal-mapped on a disk", [](Fixture &f) { f.normalMapped(); f.disk(); }, "shape 0: textured BSDFs are only supported on triangle meshes");
    refused("normal-mapped child of a blend", [](Fixture &f) {
        f.normalMapped();
        f.blends.assign(N_MATERIALS, ppg_blend{});
        ppg_blend &b = f.blends[M_OTHER];
        b.kind = 1; b.n = 2; b.child[0] = M_DIFFUSE; b.child[1] = M_SUBJECT; b.weight[0] = 0.5f;
    }, "material 2: blend: child 1 (material 1) is masked, two-sided or bump-mapped: the adapters go around the blend, on its own record");

    refused("null two-sided", [](Fixture &f) { f.null(); f.materials[M_SUBJECT].flags = PPG_MAT_TWOSIDED; }, who + "null cannot be two-sided: only BRDFs can be (twosided.cpp:84-88)");
    refused("null masked", [](Fixture &f) { f.null(); f.materials[M_SUBJECT].flags = PPG_MAT_MASK; }, who + "null: a mask around the null BSDF is not supported");
    refused("null with another flag", [](Fixture &f) { f.null(); f.materials[M_SUBJECT].flags = PPG_MAT_NONLINEAR; }, who + "null takes no flags");
    refused("null normal-mapped", [](Fixture &f) { f.null(); f.normalMapped(); }, who + "null takes no flags");
    refused("null with a reflectance bitmap", [](Fixture &f) { f.null(); f.materials[M_SUBJECT].texture = 1u; }, who + "null reads no bitmap and takes no bump or normal map: `texture` must be 0");
    refused("null bump-mapped", [](Fixture &f) { f.null(); f.materials[M_SUBJECT].texture = 1u << 16; }, who + "null reads no bitmap and takes no bump or normal map: `texture` must be 0");
    refused("null with a specular slot", [](Fixture &f) { f.null(); f.materialTextures.assign(N_MATERIALS, ppg_material_textures{0, 0, 0, 0}); f.materialTextures[M_SUBJECT].specular = 1; },
            who + "texture slot specular: null reads no bitmap");
    refused("null with an opacity slot", [](Fixture &f) { f.null(); f.materialTextures.assign(N_MATERIALS, ppg_material_textures{0, 0, 0, 0}); f.materialTextures[M_SUBJECT].opacity = 1; },
            who + "texture slot opacity: null reads no bitmap");
    refused("null with a microfacet entry", [](Fixture &f) { f.null(); f.microfacet.assign(N_MATERIALS, ppg_microfacet{}); f.microfacet[M_SUBJECT].general = 1; f.microfacet[M_SUBJECT].alpha_v = 0.2f; },
            who + "microfacet: only roughconductor, roughdielectric and roughplastic have a microfacet distribution");
    refused("null coated", [](Fixture &f) {
        f.null();
        f.coatings.assign(N_MATERIALS, ppg_coating{});
        ppg_coating &c = f.coatings[M_SUBJECT];
        c.kind = 1; c.eta = 1.5f; c.thickness = 1.0f;
        for (int k = 0; k < 3; ++k) c.specular[k] = 1.0f;
    }, who + "coating: coating over the null BSDF is not supported");
    refused("null child of a blend", [](Fixture &f) {
        f.null();
        f.blends.assign(N_MATERIALS, ppg_blend{});
        ppg_blend &b = f.blends[M_OTHER];
        b.kind = 2; b.n = 2; b.child[0] = M_DIFFUSE; b.child[1] = M_SUBJECT; b.weight[0] = 0.5f; b.weight[1] = 0.5f;
    }, "material 2: blend: child 1 (material 1): a null child is not supported");
    refused("null as the blended record", [](Fixture &f) {
        f.null();
        f.blends.assign(N_MATERIALS, ppg_blend{});
        ppg_blend &b = f.blends[M_SUBJECT];
        b.kind = 1; b.n = 2; b.child[0] = M_DIFFUSE; b.child[1] = M_OTHER; b.weight[0] = 0.5f;
    }, who + "blend: the blended material's own record must be of type PPG_BSDF_DIFFUSE (it only carries the adapters)");
    refused("null on a sphere", [](Fixture &f) { f.null(); f.sphere(); }, "sphere: material 1: the null BSDF is only supported on triangle meshes (not on spheres, disks or cylinders)");
    refused("null on a disk", [](Fixture &f) { f.null(); f.disk(); }, "shape 0: material 1: the null BSDF is only supported on triangle meshes (not on spheres, disks or cylinders)");
    refused("a type beyond the last", [](Fixture &f) { f.materials[M_SUBJECT].type = PPG_BSDF_NULL + 1; f.onTheQuad(); }, "unsupported BSDF type");

    {   // the inputs of a refused build are untouched: with the defect taken out they build, and to the tables of a scene that never had it
        Fixture f, g;
        f.null(); f.onTheQuad(); g.null(); g.onTheQuad();
        f.materials[M_SUBJECT].flags = PPG_MAT_TWOSIDED;
        HostScene Hf, Hg, Hbad;
        std::string err;
        const int bad = buildScene(f.inputs(), Hbad, err);
        f.materials[M_SUBJECT].flags = 0;
        const int rf = buildScene(f.inputs(), Hf, err), rg = buildScene(g.inputs(), Hg, err);
        const bool same = rf == PPG_OK && rg == PPG_OK && Hf.mats.size() == Hg.mats.size() && !memcmp(Hf.mats.data(), Hg.mats.data(), Hf.mats.size() * sizeof(float4)) &&
                          Hf.tris.size() == Hg.tris.size() && !memcmp(Hf.tris.data(), Hg.tris.data(), Hf.tris.size() * sizeof(float4));
        if (bad == PPG_ERR_INVALID && same) printf("ok a refused build leaves its inputs usable\n");
        else { printf("FAILED a refused build leaves its inputs usable: %d %d %d\n", bad, rf, rg); ++failures; }
    }

    if (failures) { printf("%d check(s) FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
