/*
 * scene_build_check.hip — buildScene() (csrc/ppg_scene_build.h) without a context and without a device: one accepted scene that fills
 * every host table at once (66 triangles, cut to 64 and to 0), one refused scene per kind of index the function trusts, each at its first
 * invalid value and with its exact message, and pairs of defects whose winner is the order of ppg_set_scene's checks.  Prints an FNV-1a
 * checksum of every table of the accepted scenes.  Built with the host sanitizers and run by tests/test_scene_build.py.
 */
#include <cstdio>
#include <functional>
#include <limits>

#include "../practical-path-guiding_amd/csrc/ppg_scene_build.h"

namespace {

struct Fixture {
    std::vector<float> positions, normals, texcoords, rtrans, texels[2], envTexels;
    std::vector<uint32_t> indices, triMaterial;
    std::vector<int32_t> triEmitter;
    std::vector<ppg_material> materials;
    std::vector<ppg_emitter> emitters;
    std::vector<ppg_sphere> spheres;
    std::vector<ppg_texture> textures;
    ppg_envmap envmap{};
    ppg_scene scene{};
    std::vector<ppg_material_textures> materialTextures;
    std::vector<ppg_microfacet> microfacet;
    std::vector<ppg_coating> coatings;
    std::vector<ppg_blend> blends;
    std::vector<ppg_delta_emitter> deltaEmitters;
    std::vector<ppg_shape> shapes;
    ppg_lens lens{0.05f, 3.0f};

    // the arrays may have been changed or grown since: point the scene at them again
    SceneInputs inputs() {
        ppg_scene &s = scene;
        s.positions = positions.data(); s.normals = normals.data(); s.texcoords = texcoords.data();
        s.indices = indices.data(); s.tri_material = triMaterial.data(); s.tri_emitter = triEmitter.data();
        s.materials = materials.data(); s.emitters = emitters.data(); s.rtrans = rtrans.data();
        s.spheres = spheres.data(); s.textures = textures.data(); s.envmap = &envmap;
        for (int i = 0; i < 2; ++i) textures[i].rgb = texels[i].data();
        envmap.rgb = envTexels.data();
        return SceneInputs{&scene, materialTextures, microfacet, coatings, blends, deltaEmitters, shapes, &lens, 2e-6f, 4, false};
    }
};

enum { M_TEXTURED, M_PLAIN, M_ROUGHPLASTIC, M_ANISO, M_BLEND, M_CHILD_DIFFUSE, M_CHILD_CONDUCTOR, M_MIXTURE, M_PLASTIC, N_MATERIALS };

ppg_material material(int type, float r, float alpha = 0.0f, float eta = 0.0f) {
    ppg_material m{};
    m.type = type;
    for (int c = 0; c < 3; ++c) { m.reflectance[c] = r; m.specular[c] = 1.0f; m.eta[c] = eta; m.k[c] = type == PPG_BSDF_ROUGHCONDUCTOR ? 3.0f : 0.0f; m.opacity[c] = 0.5f; }
    m.alpha = alpha;
    return m;
}

// A strip of 33 unit quads in the plane z = 0 under every kind of light; the materials cycle over the triangles, the last quad is the
// area light.  nTris: 66, or the same scene cut to its first nTris triangles.
Fixture acceptedScene(uint32_t nTris) {
    Fixture f;
    for (int i = 0; i < 34; ++i)
        for (int j = 0; j < 2; ++j) {
            f.positions.insert(f.positions.end(), {(float)i, (float)j, 0.0f});
            f.normals.insert(f.normals.end(), {0.0f, 0.0f, 1.0f});
            f.texcoords.insert(f.texcoords.end(), {(float)i / 33.0f, (float)j});
        }
    const uint32_t cycle[5] = {M_TEXTURED, M_ROUGHPLASTIC, M_ANISO, M_BLEND, M_MIXTURE};
    for (uint32_t q = 0; q < 33; ++q) {
        const uint32_t a = 2 * q, b = 2 * q + 2, c = 2 * q + 3, d = 2 * q + 1;
        f.indices.insert(f.indices.end(), {a, b, c, a, c, d});
        for (uint32_t k = 0; k < 2; ++k) {
            const uint32_t t = 2 * q + k;
            f.triMaterial.push_back(q == 32 ? (uint32_t)M_PLAIN : cycle[t % 5]);
            f.triEmitter.push_back(q == 32 ? 0 : -1);
        }
    }
    f.materials.resize(N_MATERIALS);
    f.materials[M_TEXTURED] = material(PPG_BSDF_DIFFUSE, 0.7f);
    f.materials[M_TEXTURED].texture = 1;
    f.materials[M_PLAIN] = material(PPG_BSDF_DIFFUSE, 0.5f);
    f.materials[M_ROUGHPLASTIC] = material(PPG_BSDF_ROUGHPLASTIC, 0.4f, 0.2f, 1.5f);
    f.materials[M_ROUGHPLASTIC].rtrans = 1;
    f.materials[M_ANISO] = material(PPG_BSDF_ROUGHCONDUCTOR, 0.9f, 0.1f, 0.2f);
    f.materials[M_BLEND] = material(PPG_BSDF_DIFFUSE, 0.0f);
    f.materials[M_CHILD_DIFFUSE] = material(PPG_BSDF_DIFFUSE, 0.3f);
    f.materials[M_CHILD_CONDUCTOR] = material(PPG_BSDF_ROUGHCONDUCTOR, 0.8f, 0.3f, 0.4f);
    f.materials[M_MIXTURE] = material(PPG_BSDF_DIFFUSE, 0.0f);
    f.materials[M_PLASTIC] = material(PPG_BSDF_PLASTIC, 0.6f, 0.0f, 1.5f);
    f.emitters = {ppg_emitter{{10.0f, 9.0f, 8.0f}, 0.0f}, ppg_emitter{{3.0f, 2.0f, 1.0f}, 0.0f}};
    f.rtrans = {0.9f, 0.8f, 0.7f, 0.6f, 0.95f, 0.85f, 0.75f, 0.65f, 0.55f, 0.9f};
    f.texels[0] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f, 0.15f, 0.25f, 0.35f};
    f.texels[1] = {0.9f, 0.8f, 0.7f, 0.6f, 0.5f, 0.4f, 0.3f, 0.2f, 0.1f, 0.05f, 0.15f, 0.25f};
    f.textures.resize(2);
    for (int i = 0; i < 2; ++i) {
        ppg_texture &t = f.textures[i];
        t.width = t.height = 2;
        t.uv_scale[0] = t.uv_scale[1] = 1.0f + i;
        t.uv_offset[0] = 0.25f * i; t.uv_offset[1] = 0.0f;
        t.wrap_u = PPG_WRAP_REPEAT; t.wrap_v = i ? PPG_WRAP_CLAMP : PPG_WRAP_MIRROR;
        t.nearest = i;
    }
    for (int k = 0; k < 4 * 2 * 3; ++k) f.envTexels.push_back(0.05f + 0.03f * (float)((k * 7) % 11));
    f.envmap.width = 4; f.envmap.height = 2; f.envmap.scale = 1.5f;
    const float identity3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memcpy(f.envmap.to_world, identity3, sizeof identity3);
    ppg_sphere sp{};
    sp.center[0] = 5.0f; sp.center[1] = 0.5f; sp.center[2] = 1.0f; sp.radius = 0.5f;
    memcpy(sp.to_world, identity3, sizeof identity3);
    sp.material = M_PLAIN; sp.emitter = -1;
    f.spheres = {sp};
    ppg_shape disk{}, cyl{};
    const float diskToWorld[12] = {0.5f, 0, 0, 10.0f, 0, 0.5f, 0, 0.5f, 0, 0, 0.5f, 3.0f};
    const float cylToWorld[12] = {1, 0, 0, 20.0f, 0, 1, 0, 0.5f, 0, 0, 1, 0.5f};
    disk.type = PPG_SHAPE_DISK; memcpy(disk.to_world, diskToWorld, sizeof diskToWorld); disk.material = M_PLAIN; disk.emitter = 1; disk.flip_normals = 1;
    cyl.type = PPG_SHAPE_CYLINDER; memcpy(cyl.to_world, cylToWorld, sizeof cylToWorld); cyl.radius = 0.25f; cyl.length = 1.5f; cyl.material = M_PLAIN; cyl.emitter = -1;
    f.shapes = {disk, cyl};

    f.materialTextures.assign(N_MATERIALS, ppg_material_textures{0, 0, 0, 0});
    f.materialTextures[M_PLASTIC].specular = 1;
    f.microfacet.assign(N_MATERIALS, ppg_microfacet{});
    f.microfacet[M_ANISO].general = 1; f.microfacet[M_ANISO].alpha_v = 0.3f; f.microfacet[M_ANISO].alpha_v_texture = 2;
    f.coatings.assign(N_MATERIALS, ppg_coating{});
    ppg_coating &c = f.coatings[M_ROUGHPLASTIC];
    c.kind = 2; c.eta = 1.4f; c.thickness = 0.5f; c.alpha = 0.15f; c.distribution = 1; c.rtrans = 0;
    for (int k = 0; k < 3; ++k) { c.sigma_a[k] = 0.1f * (k + 1); c.specular[k] = 1.0f; }
    f.blends.assign(N_MATERIALS, ppg_blend{});
    ppg_blend &b = f.blends[M_BLEND];
    b.kind = 1; b.n = 2; b.child[0] = M_CHILD_DIFFUSE; b.child[1] = M_CHILD_CONDUCTOR; b.weight[0] = 0.25f; b.weight_texture = 2;
    ppg_blend &mix = f.blends[M_MIXTURE];
    mix.kind = 2; mix.n = 3; mix.child[0] = M_CHILD_DIFFUSE; mix.child[1] = M_CHILD_CONDUCTOR; mix.child[2] = M_PLASTIC;
    mix.weight[0] = 0.5f; mix.weight[1] = 0.3f; mix.weight[2] = 0.4f; mix.ensure_energy_conservation = 1;
    ppg_delta_emitter spot{}, sun{};
    spot.type = PPG_EMITTER_SPOT; spot.position[0] = 16.0f; spot.position[1] = 0.5f; spot.position[2] = 6.0f;
    memcpy(spot.to_local, identity3, sizeof identity3); spot.to_local[8] = -1.0f;
    spot.cutoff_angle = 0.5f; spot.beam_width = 0.3f;
    sun.type = PPG_EMITTER_DIRECTIONAL; sun.direction[2] = -1.0f;
    for (int k = 0; k < 3; ++k) { spot.intensity[k] = 20.0f + k; sun.intensity[k] = 1.0f + k; }
    f.deltaEmitters = {spot, sun};

    ppg_scene &s = f.scene;
    s.n_vertices = 68; s.n_triangles = nTris; s.n_materials = N_MATERIALS; s.n_emitters = 2;
    s.n_rtrans = 2; s.rtrans_samples = 4; s.n_spheres = 1; s.n_textures = 2;
    const float c2w[16] = {1, 0, 0, 16.0f, 0, 1, 0, 0.5f, 0, 0, 1, 5.0f, 0, 0, 0, 1};
    const float s2c[16] = {1, 0, 0, -0.5f, 0, 1, 0, -0.5f, 0, 0, 1, 0, 0, 0, 1, 0};
    memcpy(s.camera.camera_to_world, c2w, sizeof c2w); memcpy(s.camera.sample_to_camera, s2c, sizeof s2c);
    s.camera.near_clip = 0.1f; s.camera.far_clip = 100.0f; s.camera.width = 32; s.camera.height = 32;
    return f;
}

int failures = 0;

template <typename T> void checksum(const char *name, const std::vector<T> &v) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    printf("  %-14s %6zu %016llx\n", name, v.size(), (unsigned long long)h);
}

void accepted(uint32_t nTris) {
    Fixture f = acceptedScene(nTris);
    HostScene H;
    std::string err;
    const int rc = buildScene(f.inputs(), H, err);
    if (rc != PPG_OK) { printf("FAILED accepted scene of %u triangles: refused: %s\n", nTris, err.c_str()); ++failures; return; }
    const DevScene &S = H.scene;
    printf("accepted %u triangles: fullMaterials %d nMaterials %u ldsNodes %d ldsTris %d small_n %d %d %d n_top %d has_null %d\n", nTris, (int)H.fullMaterials,
           H.nMaterials, H.ldsNodes, H.ldsTris, S.small_n[0], S.small_n[1], S.small_n[2], S.n_top, S.has_null);
    checksum("tris", H.tris); checksum("accel", H.accel); checksum("accelSmall", H.accelSmall); checksum("normals", H.normals); checksum("uvs", H.uvs);
    checksum("nodes", H.nodes); checksum("nodes4q", H.nodes4q); checksum("topCut", H.topCut);
    checksum("mats", H.mats); checksum("ems", H.ems); checksum("mfd", H.mfd); checksum("coat", H.coat); checksum("blend", H.blend);
    for (size_t i = 0; i < H.texTexels.size(); ++i) checksum(("texels" + std::to_string(i)).c_str(), H.texTexels[i]);
    checksum("textures", H.textures);
    checksum("envTexels", H.envTexels); checksum("envCdfRows", H.envCdfRows); checksum("envCdfCols", H.envCdfCols); checksum("envRowWeights", H.envRowWeights);
    checksum("emSel", H.emSel); checksum("emArea", H.emArea); checksum("emInfo", H.emInfo); checksum("emTris", H.emTris); checksum("emNormals", H.emNormals);
    checksum("delta", H.delta); checksum("shapes", H.shapes); checksum("spheres", H.spheres); checksum("rtrans", H.rtrans);
    const std::vector<float> boxes = {H.geomMin[0], H.geomMin[1], H.geomMin[2], H.geomMax[0], H.geomMax[1], H.geomMax[2],
                                      H.aabbMin[0], H.aabbMin[1], H.aabbMin[2], H.aabbMax[0], H.aabbMax[1], H.aabbMax[2]};
    checksum("boxes", boxes);
    const std::vector<float> scalars = {S.env.x, S.env.y, S.env.z, S.env.w, S.bsphere.x, S.bsphere.y, S.bsphere.z, S.bsphere.w, S.dir_sphere.x, S.dir_sphere.y,
                                        S.dir_sphere.z, S.dir_sphere.w, S.em_sel_norm, S.em_norm, S.em_scale, S.em_px, S.em_py, S.cam.inv_w, S.cam.inv_h,
                                        S.cam.aperture, S.cam.focus, (float)S.n_tris, (float)S.n_spheres, (float)S.n_shapes, (float)S.n_delta,
                                        (float)S.n_emitters, (float)S.em_w, (float)S.em_h, (float)S.rtrans_n, (float)S.cam.lens};
    checksum("scalars", scalars);
    // what the accepted scene must have filled
    const bool all = !H.mfd.empty() && !H.coat.empty() && !H.blend.empty() && H.textures.size() == 2 && !H.envTexels.empty() && !H.delta.empty() &&
                     H.shapes.size() == 2 * PPG_SHAPE_STRIDE && H.spheres.size() == 4 && !H.rtrans.empty() && H.fullMaterials &&
                     (nTris == 0 || (!H.normals.empty() && !H.uvs.empty())) && (S.small_n[0] + S.small_n[1] + S.small_n[2] == (nTris <= 64 ? (int)nTris : 0));
    if (!all) { printf("FAILED accepted scene of %u triangles: a table is missing\n", nTris); ++failures; }
}

void refused(const char *name, const std::function<void(Fixture &)> &spoil, const std::string &message) {
    Fixture f = acceptedScene(66);
    spoil(f);
    HostScene H;
    std::string err;
    const int rc = buildScene(f.inputs(), H, err);
    if (rc == PPG_ERR_INVALID && err == message) { printf("ok %s\n", name); return; }
    printf("FAILED %s: code %d, message \"%s\", expected \"%s\"\n", name, rc, err.c_str(), message.c_str());
    ++failures;
}

std::string listMessage(const char *name, size_t n) {
    return std::string(name) + ": the list has " + std::to_string(n) + " entries, the scene " + std::to_string((int)N_MATERIALS) + " materials";
}

}  // namespace

int main() {
    accepted(66);
    accepted(64);
    accepted(0);

    const uint32_t NM = N_MATERIALS, NT = 2, NE = 2, NV = 68, NR = 2;
    const std::string M = std::to_string(NM);
    refused("triangle material == n_materials", [&](Fixture &f) { f.triMaterial[0] = NM; }, "index out of range");
    refused("tri_emitter == n_emitters", [&](Fixture &f) { f.triEmitter[0] = (int32_t)NE; }, "index out of range");
    refused("vertex index == n_vertices", [&](Fixture &f) { f.indices[0] = NV; }, "vertex index out of range");
    refused("material.texture low half", [&](Fixture &f) { f.materials[M_TEXTURED].texture = NT + 1; }, "material.texture: index out of range");
    refused("material.texture high half", [&](Fixture &f) { f.materials[M_TEXTURED].texture = (NT + 1) << 16; }, "material.texture: index out of range");
    refused("specular slot", [&](Fixture &f) { f.materialTextures[M_PLASTIC].specular = NT + 1; }, "material 8: texture slot specular: index out of range");
    refused("alpha slot", [&](Fixture &f) { f.materialTextures[M_CHILD_CONDUCTOR].alpha = NT + 1; }, "material 6: texture slot alpha: index out of range");
    refused("opacity slot", [&](Fixture &f) { f.materialTextures[M_TEXTURED].opacity = NT + 1; }, "material 0: texture slot opacity: index out of range");
    refused("alpha_v_texture", [&](Fixture &f) { f.microfacet[M_ANISO].alpha_v_texture = NT + 1; }, "material 3: microfacet: alpha_v_texture: index out of range");
    refused("weight_texture", [&](Fixture &f) { f.blends[M_BLEND].weight_texture = NT + 1; }, "material 4: blend: weight_texture: index out of range");
    refused("blend child == n_materials", [&](Fixture &f) { f.blends[M_BLEND].child[1] = NM; }, "material 4: blend: child 1 (material " + M + "): index out of range");
    refused("roughplastic rtrans == n_rtrans", [&](Fixture &f) { f.materials[M_ROUGHPLASTIC].rtrans = (int32_t)NR; }, "roughplastic: material.rtrans is not a slice of scene.rtrans");
    refused("roughcoating rtrans == n_rtrans", [&](Fixture &f) { f.coatings[M_ROUGHPLASTIC].rtrans = (int32_t)NR; }, "material 2: coating: rtrans is not a slice of scene.rtrans");
    refused("sphere material", [&](Fixture &f) { f.spheres[0].material = NM; }, "index out of range");
    refused("sphere emitter", [&](Fixture &f) { f.spheres[0].emitter = (int32_t)NE; }, "index out of range");
    refused("shape material", [&](Fixture &f) { f.shapes[1].material = NM; }, "shape 1: material index out of range");
    refused("shape emitter", [&](Fixture &f) { f.shapes[1].emitter = (int32_t)NE; }, "shape 1: emitter index out of range");
    for (const size_t n : {(size_t)NM - 1, (size_t)NM + 1}) {
        refused("material textures list length", [&](Fixture &f) { f.materialTextures.resize(n); }, listMessage("material textures", n));
        refused("microfacet list length", [&](Fixture &f) { f.microfacet.resize(n); }, listMessage("microfacet", n));
        refused("coatings list length", [&](Fixture &f) { f.coatings.resize(n); }, listMessage("coatings", n));
        refused("blends list length", [&](Fixture &f) { f.blends.resize(n); }, listMessage("blends", n));
    }
    // triangle 2 is the first with the anisotropic material
    refused("NaN texcoord under an anisotropic material", [&](Fixture &f) { f.texcoords[2 * f.indices[3 * 2]] = std::numeric_limits<float>::quiet_NaN(); },
            "triangle 2: material 3: anisotropic microfacet distribution: the mesh is missing texture coordinates! The tangent space cannot be computed");

    // Two defects in one scene: the one reported is the one ppg_set_scene meets first — the triangles' references before the spheres, the
    // extent (with the BVH build) before the materials, the microfacet list before the coatings.
    refused("bad triangle material and bad sphere radius", [&](Fixture &f) { f.triMaterial[5] = NM; f.spheres[0].radius = 0.0f; }, "index out of range");
    refused("extent and plastic with eta 0", [&](Fixture &f) { f.positions[0] = -2e9f; f.materials[M_PLASTIC].eta[0] = 0.0f; }, "scene extent of 1e9 units or more (or not finite)");
    refused("microfacet and coatings list lengths", [&](Fixture &f) { f.microfacet.resize(NM - 1); f.coatings.resize(NM + 1); }, listMessage("microfacet", NM - 1));

    if (failures) { printf("%d check(s) FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
