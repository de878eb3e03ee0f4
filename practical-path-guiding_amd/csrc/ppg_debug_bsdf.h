/*
 * ppg_debug_bsdf.h — the lane of ppg_debug_bsdf / ppg_debug_bsdf_as (include/ppg_testhooks.h): one item through the BSDF layer as THIS
 * translation unit compiled it.  Included by the TRACE unit of every family (ppg_debug_kernels.h) and by the 0-SHADE_COMMON unit
 * (ppg_inst.hip), whose Mat has another layout (PPG_PARAM_TEXTURES = 0) and whose mat_spec_lum is computed: every function here is inlined
 * into the kernel that calls it, no Mat crosses a unit.
 */
#ifndef PPG_DEBUG_BSDF_H
#define PPG_DEBUG_BSDF_H

#include "../../include/ppg_testhooks.h"
#include "ppg_kernels.h"

// what the render derives from the material beside the BSDF values (shade_one: guided or not, ref_n, the search through null surfaces)
D int debug_bsdf_flag_bits(bool smooth, bool backside, bool has_null) { return (smooth ? 1 : 0) | (backside ? 2 : 0) | (has_null ? 4 : 0); }

// The FULL material as shade_one prepares it at a hit with texture coordinates uv, then mat_eval / mat_pdf / mat_sample.  A unit compiled
// with PPG_PARAM_TEXTURES = 0 looks up no bitmap on specular / alpha / opacity, as its k_shade never does.
D ppg_debug_bsdf_out debug_bsdf_full(const DevScene &S, const ppg_debug_bsdf_item &it) {
    Mat M = load_material(S, it.material);
    const unsigned int tex = __float_as_uint(S.materials[PPG_MAT_STRIDE * (size_t)it.material + 5].x);
    if (tex & 0xffffu) M.refl = tex_eval(S.textures[(tex & 0xffffu) - 1u], it.uv[0], it.uv[1]);
#if PPG_PARAM_TEXTURES
    mat_apply_textures(S, it.material, it.uv[0], it.uv[1], M);
#endif
#if PPG_MFD
    mat_apply_mfd_textures(S, it.material, it.uv[0], it.uv[1], M);
#endif
#if PPG_BLEND
    M.bu = it.uv[0]; M.bv = it.uv[1];
#endif
    const F3 wi = f3(it.wi[0], it.wi[1], it.wi[2]), wo = f3(it.wo[0], it.wo[1], it.wo[2]);
    ppg_debug_bsdf_out r;
    memset(&r, 0, sizeof r);
    const F3 f = mat_eval(M, wi, wo MAT_SCENE_ARG);
    r.eval[0] = f.x; r.eval[1] = f.y; r.eval[2] = f.z;
    r.pdf = mat_pdf(M, wi, wo MAT_SCENE_ARG);
    F3 swo;
    float spdf, seta;
    bool delta, isnull;
    unsigned int dim = 0;
    const F3 w = mat_sample(M, wi, it.sample[0], it.sample[1], swo, spdf, delta, seta, isnull, it.key, dim MAT_SCENE_ARG);
    r.wo[0] = swo.x; r.wo[1] = swo.y; r.wo[2] = swo.z;
    r.sampled_pdf = spdf;
    r.weight[0] = w.x; r.weight[1] = w.y; r.weight[2] = w.z;
    r.eta = seta; r.delta = delta ? 1 : 0; r.is_null = isnull ? 1 : 0;
    r._pad[0] = debug_bsdf_flag_bits(mat_is_smooth(M), mat_backside_or_transmission(M), mat_has_null(M));
    return r;
}

#endif
