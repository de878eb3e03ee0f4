/*
 * scene_file.h — the .ppgs container: the flat binary scene that ppg_host.scenes.save_scene() and `ppg_render --ppgs` write and that
 * both read back.  THE description of the format; ppg_host/scenes.py holds the same table in Python.  Little endian, no padding:
 *
 *   "PPGS", 6 x uint32 {n_vertices, n_triangles, n_materials, n_emitters, has_normals, blocks}
 *   positions (n_vertices x 3 floats), [normals, likewise], indices (n_triangles x 3 uint32), tri_material (uint32 each), tri_emitter
 *   (int32 each), materials (ppg_material each), emitters (ppg_emitter each), camera (ppg_camera)
 *   then, in the order of their bits, the optional blocks whose bit is set in `blocks` (a bit above 13 is refused):
 *     0 environment        3 floats: the constant environment emitter's radiance
 *     1 rtrans             2 x uint32 {n_slices, samples >= 2}, n_slices x (samples + 1) floats
 *     2 spheres            counted: uint32 n, n x ppg_sphere
 *     3 envmap             2 x uint32 {width, height}, float scale, 9 floats to_world, height x width x 3 floats
 *     4 texcoords          n_vertices x 2 floats (NaN rows: vertices of meshes without texture coordinates)
 *     5 textures           uint32 n, per texture 2 x uint32 {width, height}, 4 floats uv scale / offset, 3 x int32 {wrap_u, wrap_v, nearest},
 *                          uint32 storage, pixels: storage 0 float32 RGB, 1 uint8 sRGB-encoded RGB (decoded on load with the exact 256-entry
 *                          table of the 8-bit -> float conversion; written by the Python side only)
 *     6 rfilter            ppg_rfilter — only for a film filter other than the default box
 *     7 lens               ppg_lens — only for a thin-lens camera
 *     8 delta emitters     counted: ppg_delta_emitter (point / spot / directional)
 *     9 material textures  per material: n_materials x ppg_material_textures — only when a material has a bitmap on specular / alpha / opacity
 *    10 shapes             counted: ppg_shape (analytic disks and cylinders)
 *    11 microfacet         per material: ppg_microfacet — only when a material states alphaU / alphaV, phong or sampleVisible = false
 *    12 coatings           per material: ppg_coating — only when a material has a coating / roughcoating
 *    13 blends             per material: ppg_blend — only when a material is a blendbsdf / mixturebsdf; its children are materials of the list
 *   A counted or per-material block is written only when its list is not empty; images are 0 < width, height < 32768.
 *
 * Needs SceneData and the standard library: no HIP, nothing of the driver (tests/scene_file_check.cpp runs it under the sanitizers).
 */
#ifndef PPG_SCENE_FILE_H
#define PPG_SCENE_FILE_H

#include <cmath>
#include <cstring>
#include <fstream>
#include <istream>
#include <ostream>
#include <vector>

#include "scene_data.h"

namespace ppg {
namespace scene_file {

enum Bit : uint32_t {
    ENVIRONMENT = 1u << 0, RTRANS = 1u << 1, SPHERES = 1u << 2, ENVMAP = 1u << 3, TEXCOORDS = 1u << 4, TEXTURES = 1u << 5, RFILTER = 1u << 6,
    LENS = 1u << 7, DELTA_EMITTERS = 1u << 8, MATERIAL_TEXTURES = 1u << 9, SHAPES = 1u << 10, MICROFACET = 1u << 11, COATINGS = 1u << 12,
    BLENDS = 1u << 13, N_BITS = 14
};

// Every count read from the file is checked against what is left of it before anything is sized by it: a corrupt or truncated file is
// refused, never an allocation of whatever size its header claims.
struct Reader {
    std::istream &f;
    uint64_t size;
    bool fits(uint64_t bytes) { const std::streamoff p = f.tellg(); return p >= 0 && bytes <= size - (uint64_t)p; }
    bool raw(void *to, uint64_t bytes) { return fits(bytes) && f.read((char *)to, (std::streamsize)bytes); }
    template <class T> bool array(std::vector<T> &v, uint64_t n) {
        if (n > size || !fits(n * sizeof(T))) return false;
        v.resize((size_t)n);
        return (bool)f.read((char *)v.data(), (std::streamsize)(n * sizeof(T)));
    }
    bool imageSize(uint32_t wh[2]) { return raw(wh, 8) && wh[0] > 0 && wh[1] > 0 && wh[0] <= 0x7fffu && wh[1] <= 0x7fffu; }  // what ppg_set_scene accepts
};
struct Writer {
    std::ostream &f;
    void raw(const void *from, size_t bytes) { f.write((const char *)from, (std::streamsize)bytes); }
    template <class T> void array(const std::vector<T> &v) { raw(v.data(), v.size() * sizeof(T)); }
};

struct Block {
    uint32_t bit;
    bool (*present)(const SceneData &);
    void (*write)(Writer &, const SceneData &);
    bool (*read)(Reader &, SceneData &);
};

// uint32 n, n x T
template <class T, std::vector<T> SceneData::*list> Block counted(uint32_t bit) {
    return {bit, [](const SceneData &s) { return !(s.*list).empty(); },
            [](Writer &w, const SceneData &s) { const uint32_t n = (uint32_t)(s.*list).size(); w.raw(&n, 4); w.array(s.*list); },
            [](Reader &r, SceneData &s) { uint32_t n = 0; return r.raw(&n, 4) && r.array(s.*list, n); }};
}
// n_materials x T
template <class T, std::vector<T> SceneData::*list> Block perMaterial(uint32_t bit) {
    return {bit, [](const SceneData &s) { return !(s.*list).empty(); },
            [](Writer &w, const SceneData &s) { w.array(s.*list); },
            [](Reader &r, SceneData &s) { return r.array(s.*list, s.materials.size()); }};
}

inline const std::vector<Block> &blocks() {
    static const std::vector<Block> table = {
        {ENVIRONMENT, [](const SceneData &s) { return s.hasEnvironment; },
         [](Writer &w, const SceneData &s) { w.raw(s.environment, 12); },
         [](Reader &r, SceneData &s) { s.hasEnvironment = true; return r.raw(s.environment, 12); }},
        {RTRANS, [](const SceneData &s) { return !s.rtrans.empty(); },
         [](Writer &w, const SceneData &s) {
             const uint32_t rt[2] = {(uint32_t)(s.rtrans.size() / (s.rtransSamples + 1)), s.rtransSamples};
             w.raw(rt, 8); w.array(s.rtrans);
         },
         [](Reader &r, SceneData &s) {
             uint32_t rt[2];
             if (!r.raw(rt, 8) || rt[1] < 2) return false;
             s.rtransSamples = rt[1];
             return r.array(s.rtrans, (uint64_t)rt[0] * ((uint64_t)rt[1] + 1));
         }},
        counted<ppg_sphere, &SceneData::spheres>(SPHERES),
        {ENVMAP, [](const SceneData &s) { return s.hasEnvmap; },
         [](Writer &w, const SceneData &s) {
             const uint32_t wh[2] = {s.envmap.width, s.envmap.height};
             w.raw(wh, 8); w.raw(&s.envmap.scale, 4); w.raw(s.envmap.to_world, 36); w.array(s.envmapRgb);
         },
         [](Reader &r, SceneData &s) {
             uint32_t wh[2];
             if (!r.imageSize(wh) || !r.raw(&s.envmap.scale, 4) || !r.raw(s.envmap.to_world, 36)) return false;
             s.envmap.width = wh[0]; s.envmap.height = wh[1]; s.hasEnvmap = true;
             return r.array(s.envmapRgb, (uint64_t)wh[0] * wh[1] * 3);
         }},
        {TEXCOORDS, [](const SceneData &s) { return !s.texcoords.empty(); },
         [](Writer &w, const SceneData &s) { w.array(s.texcoords); },
         [](Reader &r, SceneData &s) { return r.array(s.texcoords, (uint64_t)(s.positions.size() / 3) * 2); }},
        {TEXTURES, [](const SceneData &s) { return !s.textures.empty(); },
         [](Writer &w, const SceneData &s) {
             const uint32_t n = (uint32_t)s.textures.size();
             w.raw(&n, 4);
             for (uint32_t k = 0; k < n; ++k) {
                 const ppg_texture &t = s.textures[k];
                 const uint32_t wh[2] = {t.width, t.height}, storage = 0;
                 const float sc[4] = {t.uv_scale[0], t.uv_scale[1], t.uv_offset[0], t.uv_offset[1]};
                 const int32_t wr[3] = {t.wrap_u, t.wrap_v, t.nearest};
                 w.raw(wh, 8); w.raw(sc, 16); w.raw(wr, 12); w.raw(&storage, 4); w.array(s.texturePixels[k]);
             }
         },
         [](Reader &r, SceneData &s) {
             uint32_t n = 0;
             if (!r.raw(&n, 4)) return false;
             float srgb[256];
             for (int i = 0; i < 256; ++i) { const double v = i / 255.0; srgb[i] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4)); }
             for (uint32_t k = 0; k < n; ++k) {
                 uint32_t wh[2], storage = 0; float sc[4]; int32_t wr[3];
                 if (!r.imageSize(wh) || !r.raw(sc, 16) || !r.raw(wr, 12) || !r.raw(&storage, 4)) return false;
                 ppg_texture t{};
                 t.width = wh[0]; t.height = wh[1]; t.uv_scale[0] = sc[0]; t.uv_scale[1] = sc[1]; t.uv_offset[0] = sc[2]; t.uv_offset[1] = sc[3];
                 t.wrap_u = wr[0]; t.wrap_v = wr[1]; t.nearest = wr[2];
                 const uint64_t floats = (uint64_t)wh[0] * wh[1] * 3;
                 std::vector<float> px;
                 if (storage == 1) {
                     std::vector<unsigned char> bytes;
                     if (!r.array(bytes, floats)) return false;
                     px.resize(bytes.size());
                     for (size_t i = 0; i < px.size(); ++i) px[i] = srgb[bytes[i]];
                 } else if (!r.array(px, floats)) return false;
                 s.textures.push_back(t); s.texturePixels.push_back(std::move(px));
             }
             return true;
         }},
        {RFILTER, [](const SceneData &s) { return s.hasRFilter; },
         [](Writer &w, const SceneData &s) { w.raw(&s.rfilter, sizeof(ppg_rfilter)); },
         [](Reader &r, SceneData &s) { s.hasRFilter = true; return r.raw(&s.rfilter, sizeof(ppg_rfilter)); }},
        {LENS, [](const SceneData &s) { return s.hasLens; },
         [](Writer &w, const SceneData &s) { w.raw(&s.lens, sizeof(ppg_lens)); },
         [](Reader &r, SceneData &s) { s.hasLens = true; return r.raw(&s.lens, sizeof(ppg_lens)); }},
        counted<ppg_delta_emitter, &SceneData::deltaEmitters>(DELTA_EMITTERS),
        perMaterial<ppg_material_textures, &SceneData::materialTextures>(MATERIAL_TEXTURES),
        counted<ppg_shape, &SceneData::shapes>(SHAPES),
        perMaterial<ppg_microfacet, &SceneData::microfacet>(MICROFACET),
        perMaterial<ppg_coating, &SceneData::coatings>(COATINGS),
        perMaterial<ppg_blend, &SceneData::blends>(BLENDS),
    };
    return table;
}

inline bool load(std::istream &f, SceneData &s) {
    f.seekg(0, std::ios::end);
    Reader r{f, f ? (uint64_t)f.tellg() : 0};
    f.seekg(0);
    char magic[4];
    uint32_t hdr[6];
    if (!r.raw(magic, 4) || memcmp(magic, "PPGS", 4) != 0 || !r.raw(hdr, sizeof hdr)) return false;
    const uint32_t nv = hdr[0], nt = hdr[1], hasN = hdr[4], flags = hdr[5];
    if (flags >> N_BITS) return false;  // a block this reader does not know
    if (!r.array(s.positions, 3 * (uint64_t)nv) || (hasN && !r.array(s.normals, 3 * (uint64_t)nv)) || !r.array(s.indices, 3 * (uint64_t)nt) ||
        !r.array(s.triMaterial, nt) || !r.array(s.triEmitter, nt) || !r.array(s.materials, hdr[2]) || !r.array(s.emitters, hdr[3]) ||
        !r.raw(&s.camera, sizeof(ppg_camera)))
        return false;
    for (const Block &b : blocks())
        if ((flags & b.bit) && !b.read(r, s)) return false;
    return (bool)f;
}

inline bool save(std::ostream &f, const SceneData &s) {
    uint32_t flags = 0;
    for (const Block &b : blocks()) if (b.present(s)) flags |= b.bit;
    const uint32_t hdr[6] = {(uint32_t)(s.positions.size() / 3), (uint32_t)(s.indices.size() / 3), (uint32_t)s.materials.size(), (uint32_t)s.emitters.size(),
                             s.normals.empty() ? 0u : 1u, flags};
    Writer w{f};
    w.raw("PPGS", 4); w.raw(hdr, sizeof hdr);
    w.array(s.positions); w.array(s.normals); w.array(s.indices); w.array(s.triMaterial); w.array(s.triEmitter); w.array(s.materials); w.array(s.emitters);
    w.raw(&s.camera, sizeof(ppg_camera));
    for (const Block &b : blocks()) if (flags & b.bit) b.write(w, s);
    return (bool)f;
}

}  // namespace scene_file

// a corrupt or truncated file is `false` ("cannot load scene"), whatever it makes the reader throw
inline bool loadScene(const char *path, SceneData &s) {
    try {
        std::ifstream f(path, std::ios::binary);
        return f && scene_file::load(f, s);
    } catch (const std::exception &) { return false; }
}
inline bool saveScene(const char *path, const SceneData &s) {
    std::ofstream f(path, std::ios::binary);
    return scene_file::save(f, s);
}

}  // namespace ppg
#endif
