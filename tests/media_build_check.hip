/*
 * media_build_check.hip — buildScene() (csrc/ppg_scene_build.h), the pure stage of ppg_set_scene, on ppg_set_media's list, without a
 * context and without a device: one accepted scene's tables — the derived sigmaT, sampling weights and `single`'s density, the binding
 * words in the kernels' primitive order —, a list that binds nothing, and every refusal of the list with its exact message.  Built with
 * the host sanitizers and run by tests/test_media.py.
 */
#include <cstdio>
#include <functional>

#include "../practical-path-guiding_amd/csrc/ppg_scene_build.h"

namespace {

struct Fixture {
    // two quads (four triangles), a sphere and a disk
    std::vector<float> positions{0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 2, 1, 0, 2, 1, 1, 2, 0, 1, 2};
    std::vector<uint32_t> indices{0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7}, triMaterial{0, 0, 0, 0};
    std::vector<int32_t> triEmitter{0, 0, -1, -1};
    std::vector<ppg_material> materials;
    std::vector<ppg_emitter> emitters{ppg_emitter{{5.0f, 5.0f, 5.0f}, 0.0f}};
    std::vector<ppg_sphere> spheres;
    ppg_scene scene{};
    std::vector<ppg_material_textures> materialTextures;
    std::vector<ppg_microfacet> microfacet;
    std::vector<ppg_coating> coatings;
    std::vector<ppg_blend> blends;
    std::vector<ppg_delta_emitter> deltaEmitters;
    std::vector<ppg_shape> shapes;
    std::vector<ppg_medium> media;
    std::vector<uint32_t> triMedia{0, 0, 0, 0}, sphereMedia{0}, shapeMedia{0};
    ppg_media list{};

    static ppg_medium medium(float a0, float a1, float a2, float s0, float s1, float s2) {
        ppg_medium m{};
        m.sigma_a[0] = a0; m.sigma_a[1] = a1; m.sigma_a[2] = a2; m.sigma_s[0] = s0; m.sigma_s[1] = s1; m.sigma_s[2] = s2;
        m.strategy = PPG_MEDIUM_BALANCE; m.channel = -1; m.sampling_weight = -1.0f; m.phase = PPG_PHASE_ISOTROPIC;
        return m;
    }
    Fixture() {
        materials.resize(1);
        materials[0] = ppg_material{};
        materials[0].type = PPG_BSDF_DIFFUSE;
        for (int c = 0; c < 3; ++c) { materials[0].reflectance[c] = 0.5f; materials[0].specular[c] = 1.0f; materials[0].eta[c] = 1.5f; materials[0].k[c] = 1.0f; }
        ppg_sphere sp{};
        sp.center[0] = 0.5f; sp.center[1] = 0.5f; sp.center[2] = 1.0f; sp.radius = 0.25f;
        sp.to_world[0] = sp.to_world[4] = sp.to_world[8] = 1.0f;
        sp.material = 0; sp.emitter = -1;
        spheres = {sp};
        ppg_shape d{};
        const float toWorld[12] = {0.25f, 0, 0, 0.5f, 0, 0.25f, 0, 0.5f, 0, 0, 0.25f, 1.5f};
        d.type = PPG_SHAPE_DISK; memcpy(d.to_world, toWorld, sizeof toWorld); d.material = 0; d.emitter = -1;
        shapes = {d};
        ppg_scene &s = scene;
        s.n_vertices = 8; s.n_triangles = 4; s.n_materials = 1; s.n_emitters = 1;
        const float c2w[16] = {1, 0, 0, 0.5f, 0, 1, 0, 0.5f, 0, 0, -1, 5.0f, 0, 0, 0, 1};
        const float s2c[16] = {1, 0, 0, -0.5f, 0, 1, 0, -0.5f, 0, 0, 1, 0, 0, 0, 1, 0};
        memcpy(s.camera.camera_to_world, c2w, sizeof c2w); memcpy(s.camera.sample_to_camera, s2c, sizeof s2c);
        s.camera.near_clip = 0.1f; s.camera.far_clip = 100.0f; s.camera.width = 8; s.camera.height = 8;
        // medium 0: coloured, albedos 0.5 / 0.8 / 0.25 -> weight 0.8; medium 1: a pure absorber -> weight 0; medium 2: single, no channel
        // stated -> the smallest sigmaT (channel 1); medium 3: albedo 0.25 everywhere -> raised to 0.5, manual
        media = {medium(1, 0.5f, 3, 1, 2, 1), medium(1, 2, 3, 0, 0, 0), medium(1, 0.5f, 1, 2, 0.25f, 2), medium(3, 3, 3, 1, 1, 1)};
        media[2].strategy = PPG_MEDIUM_SINGLE;
        media[3].strategy = PPG_MEDIUM_MANUAL; media[3].sampling_density = 1.5f; media[3].phase = PPG_PHASE_HG; media[3].g = 0.5f;
        triMedia = {0, 0, 1u | (2u << 16), 1u | (2u << 16)};  // the second quad: interior 0, exterior 1
        sphereMedia = {3u};                                  // interior 2
        shapeMedia = {4u << 16};                             // exterior 3
    }
    SceneInputs inputs() {
        ppg_scene &s = scene;
        s.positions = positions.data(); s.indices = indices.data(); s.tri_material = triMaterial.data(); s.tri_emitter = triEmitter.data();
        s.materials = materials.data(); s.emitters = emitters.data();
        s.n_spheres = (uint32_t)spheres.size(); s.spheres = spheres.empty() ? nullptr : spheres.data();
        list.n_media = (uint32_t)media.size(); list.media = media.data();
        list.n_tri_media = (uint32_t)triMedia.size(); list.tri_media = triMedia.data();
        list.n_sphere_media = (uint32_t)sphereMedia.size(); list.sphere_media = sphereMedia.data();
        list.n_shape_media = (uint32_t)shapeMedia.size(); list.shape_media = shapeMedia.data();
        SceneInputs in{&scene, materialTextures, microfacet, coatings, blends, deltaEmitters, shapes, nullptr, 2e-6f, 4, false};
        in.media = &list;
        return in;
    }
};

int failures = 0;

void check(bool ok, const char *what) {
    if (ok) { printf("ok %s\n", what); return; }
    printf("FAILED %s\n", what);
    ++failures;
}

void refused(const char *name, const std::function<void(Fixture &)> &spoil, const std::string &message) {
    Fixture f;
    spoil(f);
    HostScene H;
    std::string err;
    SceneInputs in = f.inputs();
    const int rc = buildScene(in, H, err);
    if (rc == PPG_ERR_INVALID && err == message) { printf("ok refused %s\n", name); return; }
    printf("FAILED refused %s: code %d, message \"%s\", expected \"%s\"\n", name, rc, err.c_str(), message.c_str());
    ++failures;
}

bool near(float a, float b) { return std::fabs(a - b) <= 1e-6f * std::max(1.0f, std::fabs(b)); }

}  // namespace

int main() {
    {   // the accepted scene and its tables
        Fixture f;
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        check(rc == PPG_OK, "accepted: the scene builds");
        check(H.fullMaterials && H.scene.has_null == 1, "accepted: FULL kernels, piecewise shadow segments");
        check(H.media.size() == 4 * PPG_MEDIUM_STRIDE && H.cameraMedium == 0, "accepted: four records, no sensor medium");
        if (H.media.size() == 4 * PPG_MEDIUM_STRIDE) {
            const float4 *Q = H.media.data();
            check(Q[0].x == 1 && Q[0].y == 2 && Q[0].z == 1 && Q[1].x == 2 && Q[1].y == 2.5f && Q[1].z == 4, "medium 0: sigmaS, sigmaT = sigmaA + sigmaS");
            check(near(Q[0].w, 0.8f), "medium 0: weight = the highest albedo");
            check(__builtin_bit_cast(int, Q[2].y) == PPG_MEDIUM_BALANCE && __builtin_bit_cast(int, Q[2].z) == PPG_PHASE_ISOTROPIC && Q[2].x == 0, "medium 0: balance, isotropic");
            Q += PPG_MEDIUM_STRIDE;
            check(Q[0].w == 0.0f && Q[1].x == 1 && Q[1].y == 2 && Q[1].z == 3, "medium 1: a pure absorber never scatters");
            Q += PPG_MEDIUM_STRIDE;
            check(near(Q[0].w, 2.0f / 3.0f) && Q[1].w == 0.75f && __builtin_bit_cast(int, Q[2].y) == PPG_MEDIUM_SINGLE, "medium 2: single's density = the smallest sigmaT");
            Q += PPG_MEDIUM_STRIDE;
            check(Q[0].w == 0.5f && Q[1].w == 1.5f && Q[2].x == 0.5f && __builtin_bit_cast(int, Q[2].z) == PPG_PHASE_HG, "medium 3: weight raised to 0.5, manual density, hg");
        }
        bool words = H.primMedia.size() == 6;
        for (uint32_t k = 0; words && k < 4; ++k) {  // leaf order: the word follows the triangle
            const uint32_t orig = (uint32_t)__builtin_bit_cast(int, H.tris[3 * k + 2].w);
            words = H.primMedia[k] == f.triMedia[orig];
        }
        check(words && H.primMedia[4] == 3u && H.primMedia[5] == (4u << 16), "accepted: the binding words in primitive order");
    }
    {   // single with a channel; the sensor's medium alone binds
        Fixture f;
        f.media[2].channel = 2;
        f.triMedia = {0, 0, 0, 0}; f.sphereMedia = {0}; f.shapeMedia = {0};
        f.list.camera_medium = 3;
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        check(rc == PPG_OK && H.cameraMedium == 3 && H.media.size() == 4 * PPG_MEDIUM_STRIDE && H.media[2 * PPG_MEDIUM_STRIDE + 1].w == 3.0f, "accepted: camera medium; single's stated channel");
    }
    {   // a list that binds nothing renders as no list does; so does no list
        Fixture f;
        f.triMedia = {0, 0, 0, 0}; f.sphereMedia = {0}; f.shapeMedia = {0};
        HostScene H, H0;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        SceneInputs in = f.inputs();
        in.media = nullptr;
        const int rc0 = buildScene(in, H0, err);
        check(rc == PPG_OK && rc0 == PPG_OK && H.media.empty() && H.primMedia.empty() && H.scene.has_null == H0.scene.has_null && H.fullMaterials == H0.fullMaterials,
              "accepted: a list without a binding changes nothing");
    }
    refused("reserved word of the list", [](Fixture &f) { f.list._reserved = 1; }, "media: a reserved word is not 0");
    refused("triangle count", [](Fixture &f) { f.triMedia.push_back(0); }, "media: tri_media has 5 entries, the scene 4 triangles");
    refused("sphere count", [](Fixture &f) { f.sphereMedia.clear(); f.sphereMedia = {0, 0}; }, "media: sphere_media has 2 entries, the scene 1 spheres");
    refused("shape count", [](Fixture &f) { f.shapeMedia = {0, 0, 0}; }, "media: shape_media has 3 entries, the scene 1 shapes");
    refused("interior index", [](Fixture &f) { f.triMedia[1] = 5; }, "media: triangle 1: medium index out of range");
    refused("exterior index", [](Fixture &f) { f.sphereMedia[0] = 5u << 16; }, "media: sphere 0: medium index out of range");
    refused("shape index", [](Fixture &f) { f.shapeMedia[0] = 9; }, "media: shape 0: medium index out of range");
    refused("camera index", [](Fixture &f) { f.list.camera_medium = 5; }, "media: camera_medium: medium index out of range");
    refused("negative coefficient", [](Fixture &f) { f.media[1].sigma_a[2] = -1.0f; }, "medium 1: a coefficient is negative");
    refused("infinite coefficient", [](Fixture &f) { f.media[0].sigma_s[0] = INFINITY; }, "medium 0: a coefficient is not finite");
    refused("NaN coefficient", [](Fixture &f) { f.media[0].sigma_a[1] = NAN; }, "medium 0: a coefficient is not finite");
    refused("reserved word of a medium", [](Fixture &f) { f.media[3]._reserved[2] = 7; }, "medium 3: a reserved word is not 0");
    refused("strategy", [](Fixture &f) { f.media[0].strategy = 3; }, "medium 0: unknown sampling strategy");
    refused("phase", [](Fixture &f) { f.media[0].phase = 2; }, "medium 0: unknown phase function");
    refused("g = 1", [](Fixture &f) { f.media[3].g = 1.0f; }, "medium 3: hg: g must lie in (-1, 1)");
    refused("g NaN", [](Fixture &f) { f.media[3].g = NAN; }, "medium 3: hg: g must lie in (-1, 1)");
    refused("weight", [](Fixture &f) { f.media[0].sampling_weight = 1.5f; }, "medium 0: mediumSamplingWeight must lie in [0, 1] (or be -1: derive it)");
    refused("negative weight", [](Fixture &f) { f.media[0].sampling_weight = -0.5f; }, "medium 0: mediumSamplingWeight must lie in [0, 1] (or be -1: derive it)");
    refused("channel", [](Fixture &f) { f.media[2].channel = 3; }, "medium 2: single: channel must be 0, 1 or 2 (or negative: the smallest sigmaT)");
    refused("manual density", [](Fixture &f) { f.media[3].sampling_density = 0.0f; }, "medium 3: manual: samplingDensity must be finite and > 0");
    {   // 65536 media
        Fixture f;
        f.media.assign(65536, Fixture::medium(1, 1, 1, 1, 1, 1));
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        check(rc == PPG_ERR_INVALID && err == "media: 65536 media, at most 65535 are supported", "refused: more than 65535 media");
    }
    {   // a refused list leaves the inputs as they were: they build once the defect is taken out
        Fixture f;
        f.triMedia[1] = 5;
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        f.triMedia[1] = 0;
        const int rc2 = buildScene(f.inputs(), H, err);
        check(rc == PPG_ERR_INVALID && rc2 == PPG_OK && H.primMedia.size() == 6, "a refused list builds once its defect is taken out");
    }
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
