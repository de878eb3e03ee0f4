/*
 * hetmedia_build_check.hip — buildScene() (csrc/ppg_scene_build.h), the pure stage of ppg_set_scene, on ppg_set_media_volumes' list, without
 * a context and without a device: one accepted scene's tables — worldToGrid, the world box, maxDensity's inverse on a hand-computed case,
 * the default box of a const density —, a list whose media no primitive binds, and every refusal of the list with its exact message.
 * Built with the host sanitizers and run by tests/test_hetmedia.py.
 */
#include <cstdio>
#include <functional>

#include "../practical-path-guiding_amd/csrc/ppg_scene_build.h"

namespace {

struct Fixture {
    // one quad (two triangles) carrying an emitter
    std::vector<float> positions{0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0};
    std::vector<uint32_t> indices{0, 1, 2, 0, 2, 3}, triMaterial{0, 0};
    std::vector<int32_t> triEmitter{0, 0};
    std::vector<ppg_material> materials;
    std::vector<ppg_emitter> emitters{ppg_emitter{{5.0f, 5.0f, 5.0f}, 0.0f}};
    ppg_scene scene{};
    std::vector<ppg_material_textures> materialTextures;
    std::vector<ppg_microfacet> microfacet;
    std::vector<ppg_coating> coatings;
    std::vector<ppg_blend> blends;
    std::vector<ppg_delta_emitter> deltaEmitters;
    std::vector<ppg_shape> shapes;
    std::vector<ppg_medium> media;
    std::vector<uint32_t> triMedia{1u, 1u};  // interior 0
    ppg_media list{};
    // volume 0: a 3 x 2 x 2 density grid over [0, 4] x [0, 1] x [0, 2], turned a quarter about z, scaled by 2 and moved to (10, 20, 30);
    // 1: a 2 x 2 x 2 RGB grid; 2: a const density 0.25; 3: a const albedo
    std::vector<float> density, albedo;
    std::vector<ppg_volume> volumes;
    std::vector<ppg_medium_volumes> entries;
    ppg_media_volumes vlist{};

    static ppg_medium plain() {
        ppg_medium m{};
        m.channel = -1; m.sampling_weight = -1.0f;
        return m;
    }
    Fixture() {
        materials.resize(1);
        materials[0] = ppg_material{};
        materials[0].type = PPG_BSDF_DIFFUSE;
        for (int c = 0; c < 3; ++c) { materials[0].reflectance[c] = 0.5f; materials[0].specular[c] = 1.0f; materials[0].eta[c] = 1.5f; materials[0].k[c] = 1.0f; }
        ppg_scene &s = scene;
        s.n_vertices = 4; s.n_triangles = 2; s.n_materials = 1; s.n_emitters = 1;
        const float c2w[16] = {1, 0, 0, 0.5f, 0, 1, 0, 0.5f, 0, 0, -1, 5.0f, 0, 0, 0, 1};
        const float s2c[16] = {1, 0, 0, -0.5f, 0, 1, 0, -0.5f, 0, 0, 1, 0, 0, 0, 1, 0};
        memcpy(s.camera.camera_to_world, c2w, sizeof c2w); memcpy(s.camera.sample_to_camera, s2c, sizeof s2c);
        s.camera.near_clip = 0.1f; s.camera.far_clip = 100.0f; s.camera.width = 8; s.camera.height = 8;
        media = {plain(), plain(), plain()};
        media[1].phase = PPG_PHASE_HG; media[1].g = 0.5f;
        media[2].sigma_a[0] = media[2].sigma_a[1] = media[2].sigma_a[2] = 1.0f;  // a homogeneous one, named by no entry
        density.assign(12, 0.5f); density[5] = 1.0f; density[7] = 0.0f;
        albedo.assign(24, 0.25f);
        ppg_volume g{};
        g.kind = PPG_VOLUME_GRID; g.channels = 1; g.res[0] = 3; g.res[1] = 2; g.res[2] = 2;
        g.aabb_max[0] = 4.0f; g.aabb_max[1] = 1.0f; g.aabb_max[2] = 2.0f;
        const float quarter[16] = {0, -2, 0, 10, 2, 0, 0, 20, 0, 0, 2, 30, 0, 0, 0, 1};
        memcpy(g.to_world, quarter, sizeof quarter);
        ppg_volume a{};
        a.kind = PPG_VOLUME_GRID; a.channels = 3; a.res[0] = a.res[1] = a.res[2] = 2;
        a.aabb_min[0] = a.aabb_min[1] = a.aabb_min[2] = -1.0f; a.aabb_max[0] = a.aabb_max[1] = a.aabb_max[2] = 1.0f;
        a.to_world[0] = a.to_world[5] = a.to_world[10] = a.to_world[15] = 1.0f;
        ppg_volume cd{};
        cd.kind = PPG_VOLUME_CONST; cd.channels = 1; cd.value[0] = 0.25f;
        ppg_volume ca{};
        ca.kind = PPG_VOLUME_CONST; ca.channels = 3; ca.value[0] = 0.9f; ca.value[1] = 0.5f; ca.value[2] = 0.0f;
        volumes = {g, a, cd, ca};
        entries = {ppg_medium_volumes{0, 0, 1, 8.0f, {0, 0, 0, 0}}, ppg_medium_volumes{1, 2, 3, 2.0f, {0, 0, 0, 0}}};
    }
    SceneInputs inputs() {
        ppg_scene &s = scene;
        s.positions = positions.data(); s.indices = indices.data(); s.tri_material = triMaterial.data(); s.tri_emitter = triEmitter.data();
        s.materials = materials.data(); s.emitters = emitters.data();
        list.n_media = (uint32_t)media.size(); list.media = media.data();
        list.n_tri_media = (uint32_t)triMedia.size(); list.tri_media = triMedia.data();
        volumes[0].data = density.empty() ? nullptr : density.data(); volumes[1].data = albedo.data();
        vlist.n_volumes = (uint32_t)volumes.size(); vlist.volumes = volumes.data();
        vlist.n_entries = (uint32_t)entries.size(); vlist.entries = entries.data();
        SceneInputs in{&scene, materialTextures, microfacet, coatings, blends, deltaEmitters, shapes, nullptr, 2e-6f, 4, false};
        in.media = media.empty() ? nullptr : &list;
        in.mediaVolumes = &vlist;
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
int bits(float v) { return __builtin_bit_cast(int, v); }

}  // namespace

int main() {
    {   // the accepted scene and its tables
        Fixture f;
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        check(rc == PPG_OK, "accepted: the scene builds");
        check(H.volumes.size() == 4 * PPG_VOLUME_STRIDE && H.het.size() == 3 * PPG_HET_STRIDE && H.volPool.size() == 36, "accepted: four volumes, three records, both grids' floats");
        if (H.volumes.size() == 4 * PPG_VOLUME_STRIDE && H.het.size() == 3 * PPG_HET_STRIDE) {
            const float4 *V = H.volumes.data();
            check(bits(V[0].x) == (PPG_VOLUME_GRID | (1 << 8)) && bits(V[0].y) == 3 && bits(V[0].z) == 2 && bits(V[0].w) == 2 && bits(V[4].w) == 0, "volume 0: a grid, one channel, 3 x 2 x 2, first in the pool");
            // world = (10 - 2 y, 20 + 2 x, 30 + 2 z)  =>  x = (wy - 20) / 2, y = (10 - wx) / 2, z = (wz - 30) / 2;  grid = ((3 - 1) / 4 x, (2 - 1) / 1 y, (2 - 1) / 2 z)
            check(near(V[1].x, 0) && near(V[1].y, 0.25f) && near(V[1].z, 0) && near(V[1].w, -5.0f), "volume 0: worldToGrid row 0 = (0, 1/4, 0, -5)");
            check(near(V[2].x, -0.5f) && near(V[2].y, 0) && near(V[2].z, 0) && near(V[2].w, 5.0f), "volume 0: worldToGrid row 1 = (-1/2, 0, 0, 5)");
            check(near(V[3].x, 0) && near(V[3].y, 0) && near(V[3].z, 0.25f) && near(V[3].w, -7.5f), "volume 0: worldToGrid row 2 = (0, 0, 1/4, -7.5)");
            const float4 *A = V + PPG_VOLUME_STRIDE;
            check(bits(A[0].x) == (PPG_VOLUME_GRID | (3 << 8)) && bits(A[4].w) == 12 && near(A[1].x, 0.5f) && near(A[1].w, 0.5f), "volume 1: RGB, behind volume 0 in the pool, worldToGrid = p / 2 + 1 / 2");
            const float4 *C = V + 2 * PPG_VOLUME_STRIDE;
            check(bits(C[0].x) == (PPG_VOLUME_CONST | (1 << 8)) && C[4].x == 0.25f && bits(C[PPG_VOLUME_STRIDE].x) == (PPG_VOLUME_CONST | (3 << 8)) && C[PPG_VOLUME_STRIDE + 4].y == 0.5f, "volumes 2, 3: const values");
            const float4 *Q = H.het.data();
            // the box of the eight corners: x in 10 - 2 [0, 1], y in 20 + 2 [0, 4], z in 30 + 2 [0, 2]; maxDensity = 8 * 1
            check(bits(Q[0].x) == 1 && bits(Q[0].y) == 1 && Q[0].z == 8.0f && Q[0].w == 0.125f && Q[1].w == 8.0f, "medium 0: density volume 0, albedo volume 1, invMaxDensity = 1 / (scale * 1)");
            check(Q[1].x == 8 && Q[1].y == 20 && Q[1].z == 30 && Q[2].x == 10 && Q[2].y == 28 && Q[2].z == 34, "medium 0: the world box of the eight transformed corners");
            Q += PPG_HET_STRIDE;
            check(bits(Q[0].x) == 3 && bits(Q[0].y) == 3 && Q[0].w == 2.0f && Q[1].x == INFINITY && Q[2].z == -INFINITY, "medium 1: const density: invMaxDensity = 1 / (2 * 0.25), the default box");
            Q += PPG_HET_STRIDE;
            check(bits(Q[0].x) == 0, "medium 2: homogeneous");
        }
        check(H.volPool.size() == 36 && H.volPool[5] == 1.0f && H.volPool[7] == 0.0f && H.volPool[12] == 0.25f, "accepted: the pool holds the texels in their order");
    }
    {   // heterogeneous media no primitive binds: the scene runs without the tables (a homogeneous one is bound)
        Fixture f;
        f.triMedia = {3u, 3u};
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        check(rc == PPG_OK && !H.media.empty() && H.het.empty() && H.volumes.empty() && H.volPool.empty(), "accepted: unbound heterogeneous media leave no tables");
    }
    {   // 4096 majorant free paths is the bound: a box of diagonal 6 * sqrt(..) at the largest scale that fits is accepted
        Fixture f;
        const float diag = std::sqrt(2.0f * 2.0f + 8.0f * 8.0f + 4.0f * 4.0f);
        f.entries[0].scale = 4095.9f / diag;
        HostScene H;
        std::string err;
        check(buildScene(f.inputs(), H, err) == PPG_OK, "accepted: just below 4096 majorant free paths");
    }
    refused("reserved word of the list", [](Fixture &f) { f.vlist._reserved[3] = 1; }, "media volumes: a reserved word is not 0");
    refused("no media list", [](Fixture &f) { f.media.clear(); }, "media volumes: no media list (ppg_set_media) to name a medium of");
    refused("reserved word of a volume", [](Fixture &f) { f.volumes[1]._reserved[1] = 2; }, "media volumes: volume 1: a reserved word is not 0");
    refused("kind", [](Fixture &f) { f.volumes[2].kind = 2; }, "media volumes: volume 2: unknown kind");
    refused("channels of a volume", [](Fixture &f) { f.volumes[3].channels = 2; }, "media volumes: volume 3: channels must be 1 or 3");
    refused("res", [](Fixture &f) { f.volumes[0].res[1] = 1; }, "media volumes: volume 0: a res component is below 2");
    refused("empty box", [](Fixture &f) { f.volumes[0].aabb_max[2] = 0.0f; }, "media volumes: volume 0: the data box is empty");
    refused("inverted box", [](Fixture &f) { f.volumes[1].aabb_max[0] = -2.0f; }, "media volumes: volume 1: the data box is empty");
    refused("infinite box", [](Fixture &f) { f.volumes[0].aabb_min[0] = -INFINITY; }, "media volumes: volume 0: the data box is not finite");
    refused("NaN box", [](Fixture &f) { f.volumes[0].aabb_max[1] = NAN; }, "media volumes: volume 0: the data box is not finite");
    refused("singular to_world", [](Fixture &f) { f.volumes[0].to_world[10] = 0.0f; }, "media volumes: volume 0: to_world is singular");
    refused("NaN to_world", [](Fixture &f) { f.volumes[0].to_world[3] = NAN; }, "media volumes: volume 0: to_world is not finite");
    refused("projective to_world", [](Fixture &f) { f.volumes[1].to_world[12] = 0.5f; }, "media volumes: volume 1: to_world is not affine (its last row must be 0 0 0 1)");
    refused("grid without data", [](Fixture &f) { f.density.clear(); }, "media volumes: volume 0: a grid without data");
    refused("density texel above 1", [](Fixture &f) { f.density[4] = 1.5f; }, "media volumes: volume 0: texel 4 lies outside [0, 1] or is not finite");
    refused("negative density texel", [](Fixture &f) { f.density[0] = -0.1f; }, "media volumes: volume 0: texel 0 lies outside [0, 1] or is not finite");
    refused("NaN density texel", [](Fixture &f) { f.density[11] = NAN; }, "media volumes: volume 0: texel 11 lies outside [0, 1] or is not finite");
    refused("albedo texel above 1", [](Fixture &f) { f.albedo[23] = 1.25f; }, "media volumes: volume 1: texel 23 lies outside [0, 1] or is not finite");
    refused("const value not finite", [](Fixture &f) { f.volumes[3].value[1] = INFINITY; }, "media volumes: volume 3: a value is not finite");
    refused("reserved word of an entry", [](Fixture &f) { f.entries[1]._reserved[0] = 1; }, "media volumes: entry 1: a reserved word is not 0");
    refused("medium index", [](Fixture &f) { f.entries[1].medium = 3; }, "media volumes: entry 1: medium index out of range");
    refused("density index", [](Fixture &f) { f.entries[0].density = 4; }, "media volumes: entry 0: volume index out of range");
    refused("albedo index", [](Fixture &f) { f.entries[0].albedo = 9; }, "media volumes: entry 0: volume index out of range");
    refused("a medium named twice", [](Fixture &f) { f.entries[1].medium = 0; }, "media volumes: entry 1: medium 0 is named twice");
    refused("density channels", [](Fixture &f) { f.entries[0].density = 1; }, "media volumes: entry 0: the density volume must have 1 channel");
    refused("albedo channels", [](Fixture &f) { f.entries[1].albedo = 2; }, "media volumes: entry 1: the albedo volume must have 3 channels");
    refused("scale 0", [](Fixture &f) { f.entries[0].scale = 0.0f; }, "media volumes: entry 0: scale must be finite and > 0");
    refused("scale infinite", [](Fixture &f) { f.entries[1].scale = INFINITY; }, "media volumes: entry 1: scale must be finite and > 0");
    refused("scale NaN", [](Fixture &f) { f.entries[1].scale = NAN; }, "media volumes: entry 1: scale must be finite and > 0");
    refused("const density 0", [](Fixture &f) { f.volumes[2].value[0] = 0.0f; }, "media volumes: entry 1: a const density must be finite and > 0");
    refused("const albedo above 1", [](Fixture &f) { f.volumes[3].value[0] = 1.5f; }, "media volumes: entry 1: the albedo lies outside [0, 1] or is not finite");
    refused("coefficients on a heterogeneous medium", [](Fixture &f) { f.media[0].sigma_s[1] = 0.5f; },
            "media volumes: entry 0: medium 0 states coefficients or a sampling strategy: a heterogeneous medium takes its density and albedo from volumes");
    refused("strategy on a heterogeneous medium", [](Fixture &f) { f.media[1].strategy = PPG_MEDIUM_MANUAL; f.media[1].sampling_density = 1.0f; },
            "media volumes: entry 1: medium 1 states coefficients or a sampling strategy: a heterogeneous medium takes its density and albedo from volumes");
    {   // a grid too long to track: scale * diagonal above PPG_HETMEDIUM_MAX_MEAN_STEPS
        Fixture f;
        f.entries[0].scale = 1000.0f;  // the box's diagonal is sqrt(4 + 64 + 16) = 9.165
        HostScene H;
        std::string err;
        const int rc = buildScene(f.inputs(), H, err);
        check(rc == PPG_ERR_INVALID && err.find("media volumes: entry 0: the grid is too long to track: scale times the diagonal of its world box is 9165.") == 0 &&
              err.find("majorant free paths, at most 4096 are supported") != std::string::npos, "refused: a grid too long to track");
        if (rc != PPG_ERR_INVALID || err.find("too long") == std::string::npos) printf("  (code %d, message \"%s\")\n", rc, err.c_str());
    }
    {   // a refused list leaves the inputs as they were — and an output that held the previous scene's tables keeps them
        Fixture f;
        HostScene H;
        std::string err;
        const int rc0 = buildScene(f.inputs(), H, err);
        const std::vector<float> poolBefore = H.volPool;
        f.density[4] = 2.0f;
        HostScene H2;
        const int rc = buildScene(f.inputs(), H2, err);
        f.density[4] = 0.5f;
        HostScene H3;
        const int rc2 = buildScene(f.inputs(), H3, err);
        check(rc0 == PPG_OK && rc == PPG_ERR_INVALID && H2.het.empty() && H2.volPool.empty() && H.volPool == poolBefore && rc2 == PPG_OK && H3.volPool == poolBefore,
              "a refused list leaves the previous tables in place and builds once its defect is taken out");
    }
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
