/*
 * scene_data.h — the flat scene a C++ host owns, and the one place that hands it to a context: SceneData::apply() is the call sequence
 * of the C-ABI's scene setters (include/ppg.h), used by GuidedPathTracerHIP::render (guided_path_hip.h), PluginCore::render
 * (plugin_core.h) and through them by the stand-alone driver and the Mitsuba plug-in.  Only include/ppg.h beneath it.
 */
#ifndef PPG_SCENE_DATA_H
#define PPG_SCENE_DATA_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ppg.h"

namespace ppg {

// Flat scene owned by the host (what ppg_set_scene copies from)
struct SceneData {
    std::vector<float> positions, normals;
    std::vector<uint32_t> indices, triMaterial;
    std::vector<int32_t> triEmitter;
    std::vector<ppg_material> materials;
    std::vector<ppg_emitter> emitters;
    ppg_camera camera{};
    bool hasEnvironment = false;  // constant environment emitter
    float environment[3] = {0, 0, 0};
    std::vector<float> rtrans;    // rough-transmittance slices of the roughplastic materials, rtransSamples + 1 floats each
    uint32_t rtransSamples = 0;
    std::vector<ppg_sphere> spheres;  // analytic spheres
    bool hasEnvmap = false;           // image-based environment emitter: envmap (pixels in envmapRgb)
    mutable ppg_envmap envmap{};
    std::vector<float> envmapRgb;
    std::vector<float> texcoords;                  // per-vertex texture coordinates (NaN rows: none) or empty
    mutable std::vector<ppg_texture> textures;     // bitmap textures; their pixels in texturePixels
    std::vector<std::vector<float>> texturePixels;
    bool hasRFilter = false;                       // the film's reconstruction filter (ppg_set_rfilter) when it is not the default box
    ppg_rfilter rfilter{};
    bool hasLens = false;                          // thin-lens camera (ppg_set_lens); false = pinhole
    ppg_lens lens{};
    std::vector<ppg_delta_emitter> deltaEmitters;  // point / spot / directional emitters (ppg_set_delta_emitters)
    std::vector<ppg_shape> shapes;                 // analytic disks and cylinders (ppg_set_shapes)
    // The per-material lists: each empty, or one entry per material (trimSideLists)
    std::vector<ppg_material_textures> materialTextures;  // bitmaps on specular / alpha / opacity (ppg_set_material_textures)
    std::vector<ppg_microfacet> microfacet;  // the general microfacet entries: alphaU / alphaV, phong, sampleVisible = false (ppg_set_microfacet)
    std::vector<ppg_coating> coatings;       // the coating / roughcoating adapters (ppg_set_coatings)
    std::vector<ppg_blend> blends;           // the blendbsdf / mixturebsdf combinators (ppg_set_blends)

    ppg_scene view() const {
        ppg_scene s{};
        s.n_vertices = (uint32_t)(positions.size() / 3); s.positions = positions.data();
        s.normals = normals.empty() ? nullptr : normals.data();
        s.n_triangles = (uint32_t)(indices.size() / 3); s.indices = indices.data();
        s.tri_material = triMaterial.data(); s.tri_emitter = triEmitter.data();
        s.n_materials = (uint32_t)materials.size(); s.materials = materials.data();
        s.n_emitters = (uint32_t)emitters.size(); s.emitters = emitters.data();
        s.camera = camera;
        s.environment = hasEnvironment ? environment : nullptr;
        if (hasEnvmap) { envmap.rgb = envmapRgb.data(); s.envmap = &envmap; }
        if (!spheres.empty()) { s.n_spheres = (uint32_t)spheres.size(); s.spheres = spheres.data(); }
        if (rtransSamples && !rtrans.empty()) { s.n_rtrans = (uint32_t)(rtrans.size() / (rtransSamples + 1)); s.rtrans_samples = rtransSamples; s.rtrans = rtrans.data(); }
        s.texcoords = texcoords.empty() ? nullptr : texcoords.data();
        for (size_t i = 0; i < textures.size(); ++i) textures[i].rgb = texturePixels[i].data();
        if (!textures.empty()) { s.n_textures = (uint32_t)textures.size(); s.textures = textures.data(); }
        return s;
    }

    // "One entry per material, or none": a per-material list without a live entry is cleared, one with a live entry gets materials.size()
    // entries (zero entries for the materials behind its last).  For whoever collects the entries material by material: the XML loader
    // and the Mitsuba plug-in.
    void trimSideLists() {
        trim(materialTextures, [](const ppg_material_textures &t) { return t.specular || t.alpha || t.opacity; });
        trim(microfacet, [](const ppg_microfacet &g) { return g.general != 0; });
        trim(coatings, [](const ppg_coating &c) { return c.kind != 0; });
        trim(blends, [](const ppg_blend &b) { return b.kind != 0; });
    }

    // The scene setters of the C-ABI in their one order: the side lists (ppg_set_scene consumes the context's), the scene, then the film
    // filter and the lens.  Every list is sent, so an empty one clears what the context held.  Returns the first code that is not PPG_OK
    // with the name of its call (ppg_last_error(ctx) has the message), or PPG_OK.
    struct Applied { int rc; const char *call; };
    Applied apply(ppg_ctx *ctx) const {
        const ppg_scene sv = view();
        int rc;
        if ((rc = ppg_set_delta_emitters(ctx, deltaEmitters.data(), (uint32_t)deltaEmitters.size())) != PPG_OK) return {rc, "ppg_set_delta_emitters"};
        if ((rc = ppg_set_material_textures(ctx, materialTextures.data(), (uint32_t)materialTextures.size())) != PPG_OK) return {rc, "ppg_set_material_textures"};
        if ((rc = ppg_set_shapes(ctx, shapes.data(), (uint32_t)shapes.size())) != PPG_OK) return {rc, "ppg_set_shapes"};
        if ((rc = ppg_set_microfacet(ctx, microfacet.data(), (uint32_t)microfacet.size())) != PPG_OK) return {rc, "ppg_set_microfacet"};
        if ((rc = ppg_set_coatings(ctx, coatings.data(), (uint32_t)coatings.size())) != PPG_OK) return {rc, "ppg_set_coatings"};
        if ((rc = ppg_set_blends(ctx, blends.data(), (uint32_t)blends.size())) != PPG_OK) return {rc, "ppg_set_blends"};
        if ((rc = ppg_set_scene(ctx, &sv)) != PPG_OK) return {rc, "ppg_set_scene"};  // (a cancel() during these seconds of BVH build stays set in the context)
        if ((rc = ppg_set_rfilter(ctx, hasRFilter ? &rfilter : nullptr)) != PPG_OK) return {rc, "ppg_set_rfilter"};
        if ((rc = ppg_set_lens(ctx, hasLens ? &lens : nullptr)) != PPG_OK) return {rc, "ppg_set_lens"};
        return {PPG_OK, ""};
    }

private:
    template <class T, class Live> void trim(std::vector<T> &list, Live live) {
        if (std::any_of(list.begin(), list.end(), live)) list.resize(materials.size());
        else list.clear();
    }
};

}  // namespace ppg
#endif
