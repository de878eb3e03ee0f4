/*
 * ppg_debug_kernels.h — the kernels of the test hooks (include/ppg_testhooks.h) that run the render's own device functions, included by the
 * k_trace unit of a family (ppg_inst.hip): k_debug_intersect and k_debug_sample_direct in the shapes family, which the hooks always use;
 * k_debug_bsdf in the ext family, k_debug_bsdf_coat in the coat family, which ppg_debug_bsdf uses for a scene with a coated material, and
 * k_debug_bsdf_blend in the blend family, which it uses for a scene with a blended one.
 */
#ifndef PPG_DEBUG_KERNELS_H
#define PPG_DEBUG_KERNELS_H

#include "../../include/ppg_testhooks.h"
#include "ppg_launch.h"

#if PPG_FAMILY == PPG_FAMILY_SHAPES
__global__ void k_debug_intersect(DevScene S, unsigned int n, const float4 *rays, ppg_debug_hit *out, int any) {
    extern __shared__ int dbg_stack[];
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
    const F3 o = f3(ro.x, ro.y, ro.z), d = f3(rd.x, rd.y, rd.z);
    ppg_debug_hit r;
    memset(&r, 0, sizeof r);
    r.material = -1; r.emitter = -1;
    Hit h;
    if (any) h = trace_closest4<true, true>(S, dbg_stack + threadIdx.x, (int)blockDim.x, o, d, ro.w, rd.w);
    else h = trace_closest4<false, true>(S, dbg_stack + threadIdx.x, (int)blockDim.x, o, d, ro.w, rd.w);
    r.prim = h.prim;
    if (h.prim >= 0) {
        r.t = h.t;
        if (!any) {
            Isect I;
            fill_isect_full(S, h, o, d, I);
            r.p[0] = I.p.x; r.p[1] = I.p.y; r.p[2] = I.p.z;
            r.geo_n[0] = I.geoN.x; r.geo_n[1] = I.geoN.y; r.geo_n[2] = I.geoN.z;
            r.n[0] = I.n.x; r.n[1] = I.n.y; r.n[2] = I.n.z;
            r.s[0] = I.s.x; r.s[1] = I.s.y; r.s[2] = I.s.z;
            r.wi[0] = I.wi.x; r.wi[1] = I.wi.y; r.wi[2] = I.wi.z;
            r.material = I.material; r.emitter = I.emitter;
        }
    }
    out[i] = r;
}
__global__ void k_debug_sample_direct(DevScene S, unsigned int n, const float *ref, const float *refN, const float *u, ppg_debug_direct *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DirectSample ds;
    const F3 value = emitter_sample_direct<true>(S, f3(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]), f3(refN[3 * i], refN[3 * i + 1], refN[3 * i + 2]),
                                                 u[2 * i], u[2 * i + 1], ds);
    ppg_debug_direct r;
    memset(&r, 0, sizeof r);
    const int n_sel = S.n_emitters + S.n_delta + (S.env.w != 0 ? 1 : 0);
    r.emitter = n_sel ? pmf_sample(S.em_sel_cdf, n_sel + 1, u[2 * i]) : -1;  // the choice emitter_sample_direct makes
    r.d[0] = ds.d.x; r.d[1] = ds.d.y; r.d[2] = ds.d.z; r.dist = ds.dist;
    r.n[0] = ds.n.x; r.n[1] = ds.n.y; r.n[2] = ds.n.z;
    r.pdf = ds.pdf; r.em_pdf = ds.em_pdf;
    r.value[0] = value.x; r.value[1] = value.y; r.value[2] = value.z;
    out[i] = r;
}
static void launch_debug_intersect(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_hit *out, int any) {
    hipLaunchKernelGGL(k_debug_intersect, dim3(grid), dim3(block), (size_t)PPG_LDS_STACK * block * sizeof(int), stream, S, n, rays, out, any);
}
static void launch_debug_sample_direct(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float *ref, const float *ref_n, const float *u,
                                       ppg_debug_direct *out) {
    hipLaunchKernelGGL(k_debug_sample_direct, dim3(grid), dim3(block), 0, stream, S, n, ref, ref_n, u, out);
}
#endif

#if PPG_FAMILY >= PPG_FAMILY_EXT
#if PPG_FAMILY > PPG_FAMILY_EXT
#define k_debug_bsdf PPG_FAMILY_NAME(k_debug_bsdf)  // (the ext family's is the unsuffixed one)
#endif
// ppg_debug_bsdf: the material as shade_one prepares it at a hit with texture coordinates uv, then the render's mat_eval / mat_pdf / mat_sample
__global__ void k_debug_bsdf(DevScene S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ppg_debug_bsdf_item it = items[i];
    Mat M = load_material(S, it.material);
    const unsigned int tex = __float_as_uint(S.materials[PPG_MAT_STRIDE * (size_t)it.material + 5].x);
    if (tex & 0xffffu) M.refl = tex_eval(S.textures[(tex & 0xffffu) - 1u], it.uv[0], it.uv[1]);
    mat_apply_textures(S, it.material, it.uv[0], it.uv[1], M);
    mat_apply_mfd_textures(S, it.material, it.uv[0], it.uv[1], M);
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
    out[i] = r;
}
static void launch_debug_bsdf(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    hipLaunchKernelGGL(k_debug_bsdf, dim3(grid), dim3(block), 0, stream, S, n, items, out);
}
#endif

// the hooks' launchers of this family, into its row
static void fill_debug_kernels(PathKernels &K) {
#if PPG_FAMILY == PPG_FAMILY_SHAPES
    K.debug_intersect = launch_debug_intersect;
    K.debug_sample_direct = launch_debug_sample_direct;
#endif
#if PPG_FAMILY >= PPG_FAMILY_EXT
    K.debug_bsdf = launch_debug_bsdf;
#endif
}

#endif
