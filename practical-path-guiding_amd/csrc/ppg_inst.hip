/*
 * ppg_inst.hip — one pair of instantiations of a large path kernel per translation unit (ppg_launch.h): compiled with
 * -DPPG_INST=0..1 (k_shade: NEE, both FULL settings), 2..5 (k_tail: SMALL x NEE, both FULL settings), 6 (k_commit, all six, with
 * k_commit_records and k_splat_sorted), 7 (k_shade<false, FULL, MSET_COMMON>: the common material classes of a FULL scene).
 * 8..10, compiled with -DPPG_SHAPES=1 as well: the kernels of scenes with analytic disks or cylinders (ppg_device.h PPG_SHAPES) — 8
 * k_shade_shapes<NEE, true>, 9 k_tail_shapes<false, NEE, true>, 10 k_trace_shapes<false, COUNT> and the two kernels of the test hooks
 * ppg_debug_intersect / ppg_debug_sample_direct.
 * 11..13, compiled with -DPPG_SHAPES=1 -DPPG_MFD=1: the "extended" kernels of scenes whose microfacet list has a general entry
 * (ppg_set_microfacet; ppg_device.h PPG_MFD) — 11 k_shade_ext<NEE, true>, 12 k_tail_ext<false, NEE, true>, 13 k_trace_ext<false, COUNT> (its
 * sort_slice keeps general materials out of the COMMON classes) and the kernel of the test hook ppg_debug_bsdf.
 * 14..16, compiled with -DPPG_SHAPES=1 -DPPG_MFD=1 -DPPG_COAT=1: the "coat" kernels of scenes with a coating / roughcoating
 * (ppg_set_coatings; ppg_device.h PPG_COAT) — 14 k_shade_coat<NEE, true>, 15 k_tail_coat<false, NEE, true>, 16 k_trace_coat<false, COUNT>
 * (its sort_slice keeps coated materials out of the COMMON classes too) and the hook's kernel for such a scene.  The same source as 11..13.
 */
#include <hip/hip_runtime.h>

#if defined(PPG_INST) && PPG_INST == 7
#define PPG_PARAM_TEXTURES 0  // k_shade<.., MSET_COMMON> reads no bitmap on specular / alpha / opacity (ppg_device.h mat_spec_lum)
#endif
#include "ppg_launch.h"

#ifndef PPG_INST
#error "compile with -DPPG_INST=0..16"
#endif
#if (PPG_INST >= 8) != (PPG_SHAPES != 0)
#error "units 8..16, and only they, are compiled with -DPPG_SHAPES=1"
#endif
#if (PPG_INST >= 11) != (PPG_MFD != 0)
#error "units 11..16, and only they, are compiled with -DPPG_MFD=1"
#endif
#if (PPG_INST >= 14) != (PPG_COAT != 0)
#error "units 14..16, and only they, are compiled with -DPPG_COAT=1"
#endif
#if PPG_COAT
#define ppg_launch_shade_ext ppg_launch_shade_coat
#define ppg_launch_tail_ext ppg_launch_tail_coat
#define ppg_launch_trace_ext ppg_launch_trace_coat
#define ppg_launch_debug_bsdf ppg_launch_debug_bsdf_coat
#define k_debug_bsdf k_debug_bsdf_coat
#endif

#if PPG_INST == 11 || PPG_INST == 14
void ppg_launch_shade_ext(int variant, const ShadeLaunch &a) {
    if (variant & 2)
        hipLaunchKernelGGL((k_shade<true, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
    else
        hipLaunchKernelGGL((k_shade<false, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
}
#elif PPG_INST == 12 || PPG_INST == 15
void ppg_launch_tail_ext(int variant, const TailLaunch &a) {
    if (variant & 2)
        hipLaunchKernelGGL((k_tail<false, true, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
    else
        hipLaunchKernelGGL((k_tail<false, false, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
}
#elif PPG_INST == 13 || PPG_INST == 16
#include "../../include/ppg_testhooks.h"
void ppg_launch_trace_ext(bool count, int grid, size_t lds, hipStream_t stream, const PathState &P, const DevScene &S, const Queues &Q, int qin, int lds_nodes,
                          int lds_tris, unsigned int *sorted, unsigned char *keys) {
    if (count) hipLaunchKernelGGL((k_trace<false, true>), dim3(grid), dim3(PPG_BLOCK), lds, stream, P, S, Q, qin, lds_nodes, lds_tris, sorted, keys);
    else hipLaunchKernelGGL((k_trace<false, false>), dim3(grid), dim3(PPG_BLOCK), lds, stream, P, S, Q, qin, lds_nodes, lds_tris, sorted, keys);
}
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
    const F3 wi = f3(it.wi[0], it.wi[1], it.wi[2]), wo = f3(it.wo[0], it.wo[1], it.wo[2]);
    ppg_debug_bsdf_out r;
    memset(&r, 0, sizeof r);
    const F3 f = mat_eval(M, wi, wo);
    r.eval[0] = f.x; r.eval[1] = f.y; r.eval[2] = f.z;
    r.pdf = mat_pdf(M, wi, wo);
    F3 swo;
    float spdf, seta;
    bool delta, isnull;
    unsigned int dim = 0;
    const F3 w = mat_sample(M, wi, it.sample[0], it.sample[1], swo, spdf, delta, seta, isnull, it.key, dim);
    r.wo[0] = swo.x; r.wo[1] = swo.y; r.wo[2] = swo.z;
    r.sampled_pdf = spdf;
    r.weight[0] = w.x; r.weight[1] = w.y; r.weight[2] = w.z;
    r.eta = seta; r.delta = delta ? 1 : 0; r.is_null = isnull ? 1 : 0;
    out[i] = r;
}
void ppg_launch_debug_bsdf(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    hipLaunchKernelGGL(k_debug_bsdf, dim3(grid), dim3(block), 0, stream, S, n, items, out);
}
#elif PPG_INST == 8
void ppg_launch_shade_shapes(int variant, const ShadeLaunch &a) {
    if (variant & 2)
        hipLaunchKernelGGL((k_shade<true, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
    else
        hipLaunchKernelGGL((k_shade<false, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
}
#elif PPG_INST == 9
void ppg_launch_tail_shapes(int variant, const TailLaunch &a) {
    if (variant & 2)
        hipLaunchKernelGGL((k_tail<false, true, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
    else
        hipLaunchKernelGGL((k_tail<false, false, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
}
#elif PPG_INST == 10
#include "../../include/ppg_testhooks.h"
void ppg_launch_trace_shapes(bool count, int grid, size_t lds, hipStream_t stream, const PathState &P, const DevScene &S, const Queues &Q, int qin, int lds_nodes,
                             int lds_tris, unsigned int *sorted, unsigned char *keys) {
    if (count) hipLaunchKernelGGL((k_trace<false, true>), dim3(grid), dim3(PPG_BLOCK), lds, stream, P, S, Q, qin, lds_nodes, lds_tris, sorted, keys);
    else hipLaunchKernelGGL((k_trace<false, false>), dim3(grid), dim3(PPG_BLOCK), lds, stream, P, S, Q, qin, lds_nodes, lds_tris, sorted, keys);
}
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
void ppg_launch_debug_intersect(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_hit *out, int any) {
    hipLaunchKernelGGL(k_debug_intersect, dim3(grid), dim3(block), (size_t)PPG_LDS_STACK * block * sizeof(int), stream, S, n, rays, out, any);
}
void ppg_launch_debug_sample_direct(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float *ref, const float *ref_n, const float *u,
                                    ppg_debug_direct *out) {
    hipLaunchKernelGGL(k_debug_sample_direct, dim3(grid), dim3(block), 0, stream, S, n, ref, ref_n, u, out);
}
#elif PPG_INST < 2
#define PAIR_N (PPG_INST != 0)
#define PPG_CAT2(a, b) a##b
#define PPG_CAT(a, b) PPG_CAT2(a, b)
void PPG_CAT(ppg_launch_shade_pair, PPG_INST)(int variant, const ShadeLaunch &a) {
    if (variant & 1)
        hipLaunchKernelGGL((k_shade<PAIR_N, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
    else
        hipLaunchKernelGGL((k_shade<PAIR_N, false>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
}
#elif PPG_INST < 6
#define PAIR_S (((PPG_INST - 2) & 2) != 0)
#define PAIR_N (((PPG_INST - 2) & 1) != 0)
#if PPG_INST == 2
#define PPG_TAIL_FN ppg_launch_tail_pair0
#elif PPG_INST == 3
#define PPG_TAIL_FN ppg_launch_tail_pair1
#elif PPG_INST == 4
#define PPG_TAIL_FN ppg_launch_tail_pair2
#else
#define PPG_TAIL_FN ppg_launch_tail_pair3
#endif
void PPG_TAIL_FN(int variant, const TailLaunch &a) {
    if (variant & 1)
        hipLaunchKernelGGL((k_tail<PAIR_S, PAIR_N, true>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
    else
        hipLaunchKernelGGL((k_tail<PAIR_S, PAIR_N, false>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
}
#elif PPG_INST == 7
void ppg_launch_shade_common(const ShadeLaunch &a) {
    hipLaunchKernelGGL((k_shade<false, true, MSET_COMMON>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
}
#else
void ppg_launch_commit(int sf, int df, const CommitLaunch &a) {
#define PPG_COMMIT(SFV, DFV) hipLaunchKernelGGL((k_commit<SFV, DFV>), dim3(a.grid), dim3(PPG_BLOCK), 0, a.stream, a.P, a.T, a.R, a.Q, a.nv8, a.list, a.list_n)
    if (sf == SF_NEAREST && df == DF_NEAREST) PPG_COMMIT(SF_NEAREST, DF_NEAREST);
    else if (sf == SF_NEAREST) PPG_COMMIT(SF_NEAREST, DF_BOX);
    else if (sf == SF_STOCHASTIC && df == DF_NEAREST) PPG_COMMIT(SF_STOCHASTIC, DF_NEAREST);
    else if (sf == SF_STOCHASTIC) PPG_COMMIT(SF_STOCHASTIC, DF_BOX);
    else if (df == DF_NEAREST) PPG_COMMIT(SF_BOX, DF_NEAREST);
    else PPG_COMMIT(SF_BOX, DF_BOX);
#undef PPG_COMMIT
}
void ppg_launch_commit_records(int sf, const CommitLaunch &a) {
    if (sf == SF_STOCHASTIC)
        hipLaunchKernelGGL((k_commit_records<SF_STOCHASTIC>), dim3(a.grid), dim3(PPG_BLOCK), 0, a.stream, a.P, a.T, a.R, a.Q, a.nv8, a.list, a.list_n, a.splat, a.flag_shift);
    else
        hipLaunchKernelGGL((k_commit_records<SF_NEAREST>), dim3(a.grid), dim3(PPG_BLOCK), 0, a.stream, a.P, a.T, a.R, a.Q, a.nv8, a.list, a.list_n, a.splat, a.flag_shift);
}
void ppg_launch_splat(int df, const SplatLaunch &a) {
    if (df == DF_BOX) hipLaunchKernelGGL((k_splat_sorted<DF_BOX>), dim3(a.grid), dim3(PPG_BLOCK), 0, a.stream, a.T, a.keys, a.idx, a.splat, a.n, a.leaf_bits, a.lds_nodes);
    else hipLaunchKernelGGL((k_splat_sorted<DF_NEAREST>), dim3(a.grid), dim3(PPG_BLOCK), 0, a.stream, a.T, a.keys, a.idx, a.splat, a.n, a.leaf_bits, a.lds_nodes);
}
#endif
