/*
 * ppg_debug_kernels.h — the kernels of the test hooks (include/ppg_testhooks.h) that run the render's own device functions, included by the
 * k_trace unit of a family (ppg_inst.hip): k_debug_intersect and the kernels of ppg_debug_intersect_mode in the shapes family, which the hooks always use;
 * k_debug_shading_frame in the top (lobes) family, which ppg_debug_shading_frame always uses.  Every family holds its k_debug_bsdf
 * (ppg_debug_bsdf_as; k_debug_bsdf_base .. k_debug_bsdf_lobes, the ext family's unsuffixed: ppg_debug_bsdf uses that one, or the coat / blend /
 * lobes family's for a scene that needs it), the base family also k_debug_bsdf_lean; every family holds k_debug_math_eval and
 * k_debug_math_checksum (ppg_debug_math_*): the shared float math as this module compiled it, its own out-of-line dm_ copies included;
 * and k_debug_sample_direct / k_debug_pdf_direct (ppg_debug_sample_direct_as, ppg_debug_pdf_direct): its own copy of the direct-light functions.
 */
#ifndef PPG_DEBUG_KERNELS_H
#define PPG_DEBUG_KERNELS_H

#include "../../include/ppg_mathcheck.h"
#include "../../include/ppg_testhooks.h"
#include "ppg_launch.h"
#include "ppg_debug_bsdf.h"

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
// ---- ppg_debug_intersect_mode: the other forms of the closest-hit traversal, ray by ray ----
// the record of hit h on ray (o, d); closest = false: prim and t only (any-hit)
D void debug_record(const DevScene &S, const Hit &h, F3 o, F3 d, bool closest, ppg_debug_hit *dst) {
    ppg_debug_hit r;
    memset(&r, 0, sizeof r);
    r.material = -1; r.emitter = -1;
    r.prim = h.prim;
    if (h.prim >= 0) {
        r.t = h.t;
        if (closest) {
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
    *dst = r;
}
// LANE, LANE_ANY, LANE_VOTE: trace_closest4<ANY, true, VOTE>, one ray per lane, waves of 64 (VOTE: n is a multiple of 64)
template <bool ANY, bool VOTE>
__global__ __launch_bounds__(64) void k_debug_trace_lane(DevScene S, unsigned int n, const float4 *rays, ppg_debug_hit *out) {
    extern __shared__ int dbg_stack[];
    const unsigned int i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
    const F3 o = f3(ro.x, ro.y, ro.z), d = f3(rd.x, rd.y, rd.z);
    const Hit h = trace_closest4<ANY, true, VOTE>(S, dbg_stack + threadIdx.x, 64, o, d, ro.w, rd.w);
    debug_record(S, h, o, d, !ANY, out + i);
}
// RESUME: a wave owns rays [blockIdx.x * per_wave, + per_wave) and follows k_tail's protocol: a lane without a ray takes the wave's next one,
// the lanes that hold one call trace_closest4_resume together; a lane that comes back parked keeps its ray and calls again with resume =
// true beside the other lanes' next rays.  stats[0] / [1]: rays parked at least once / twice.
__global__ __launch_bounds__(64) void k_debug_trace_resume(DevScene S, unsigned int n, const float4 *rays, ppg_debug_hit *out, int suspend_lanes, unsigned int per_wave,
                                                           unsigned int *stats) {
    extern __shared__ int dbg_stack[];
    __shared__ int park[3 * 64];
    const int lane = (int)threadIdx.x;
    unsigned int next = blockIdx.x * per_wave;
    const unsigned int end = next + per_wave < n ? next + per_wave : n;
    bool have = false, pending = false;
    unsigned int i = 0, parks = 0;
    float4 ro = make_float4(0, 0, 0, 0), rd = ro;
    Hit h;
    h.t = 0; h.u = 0; h.v = 0; h.prim = -1;
    for (;;) {
        const unsigned long long need = __ballot(!have);
        if (!have) {
            const unsigned int k = next + (unsigned int)__popcll(need & ((1ull << lane) - 1ull));
            if (k < end) { i = k; have = true; pending = false; parks = 0; ro = rays[2 * i]; rd = rays[2 * i + 1]; }
        }
        next = next + (unsigned int)__popcll(need) < end ? next + (unsigned int)__popcll(need) : end;
        if (__ballot(have) == 0ull) break;
        if (have) {
            const F3 o = f3(ro.x, ro.y, ro.z), d = f3(rd.x, rd.y, rd.z);
            pending = !trace_closest4_resume<true>(S, dbg_stack + lane, 64, o, d, ro.w, rd.w, pending, park + lane, 64, h, suspend_lanes);
            if (pending) ++parks;
            else {
                debug_record(S, h, o, d, true, out + i);
                if (parks >= 1u) atomicAdd(stats, 1u);
                if (parks >= 2u) atomicAdd(stats + 1, 1u);
                have = false;
            }
        }
    }
}
// WAVE: trace_closest4_wave<ROWS>, one ray per wave (all lanes with the same arguments); a ray it abandons (prim = -2) is walked again by
// lane 0 as k_tail walks it.  stats[0]: rays that took that way, stats[1]: the steps of the wave-wide walks (probe_steps).
template <int ROWS>
__global__ __launch_bounds__(64) void k_debug_trace_wave(DevScene S, unsigned int n, const float4 *rays, ppg_debug_hit *out, unsigned int *stats) {
    extern __shared__ int dbg_stack[];  // PPG_LDS_STACK rows of 64: the wave-wide stack (its first ROWS rows), then lane 0's column
    for (unsigned int i = blockIdx.x; i < n; i += gridDim.x) {
        const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
        const F3 o = f3(ro.x, ro.y, ro.z), d = f3(rd.x, rd.y, rd.z);
        int steps = 0;
        const Hit h = trace_closest4_wave<ROWS>(S, dbg_stack, 64, o, d, ro.w, rd.w, &steps);
        if (threadIdx.x == 0) {
            Hit hs = h;
            if (h.prim == -2) { hs = trace_closest4<false, true, false>(S, dbg_stack, 64, o, d, ro.w, rd.w); atomicAdd(stats, 1u); }
            atomicAdd(stats + 1, (unsigned int)steps);
            debug_record(S, hs, o, d, true, out + i);
        }
        __syncthreads();  // (lane 0's column is the wave-wide stack's first one)
    }
}
// KTRACE reads k_trace's P.hit: the record of hit (t, u, v, prim) on ray i
__global__ void k_debug_hit_records(DevScene S, unsigned int n, const float4 *rays, const float4 *hits, ppg_debug_hit *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1], hv = hits[i];
    Hit h;
    h.t = hv.x; h.u = hv.y; h.v = hv.z; h.prim = __float_as_int(hv.w);
    debug_record(S, h, f3(ro.x, ro.y, ro.z), f3(rd.x, rd.y, rd.z), true, out + i);
}
static void launch_debug_trace(int mode, int param, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_hit *out, unsigned int *stats) {
    const size_t lds = (size_t)PPG_LDS_STACK * 64 * sizeof(int);
    const dim3 waves((n + 63u) / 64u), block(64);
    switch (mode) {
    case PPG_DEBUG_TRACE_LANE: hipLaunchKernelGGL((k_debug_trace_lane<false, false>), waves, block, lds, stream, S, n, rays, out); break;
    case PPG_DEBUG_TRACE_LANE_ANY: hipLaunchKernelGGL((k_debug_trace_lane<true, false>), waves, block, lds, stream, S, n, rays, out); break;
    case PPG_DEBUG_TRACE_LANE_VOTE: hipLaunchKernelGGL((k_debug_trace_lane<false, true>), waves, block, lds, stream, S, n, rays, out); break;
    case PPG_DEBUG_TRACE_RESUME: {
        const unsigned int per_wave = 512;  // eight rays a lane
        hipLaunchKernelGGL(k_debug_trace_resume, dim3((n + per_wave - 1) / per_wave), block, lds, stream, S, n, rays, out, param, per_wave, stats);
        break;
    }
    case PPG_DEBUG_TRACE_WAVE: {
        const dim3 grid(n < 1024u ? n : 1024u);
        if (param == 1) hipLaunchKernelGGL((k_debug_trace_wave<1>), grid, block, lds, stream, S, n, rays, out, stats);
        else hipLaunchKernelGGL((k_debug_trace_wave<PPG_LDS_STACK>), grid, block, lds, stream, S, n, rays, out, stats);
        break;
    }
    default: break;  // (ppg_debug_intersect_mode has checked the mode)
    }
}
static void launch_debug_hit_records(hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, const float4 *hits, ppg_debug_hit *out) {
    hipLaunchKernelGGL(k_debug_hit_records, dim3((n + 63u) / 64u), dim3(64), 0, stream, S, n, rays, hits, out);
}
static void launch_debug_intersect(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_hit *out, int any) {
    hipLaunchKernelGGL(k_debug_intersect, dim3(grid), dim3(block), (size_t)PPG_LDS_STACK * block * sizeof(int), stream, S, n, rays, out, any);
}
#endif

// ---- ppg_debug_bsdf(_as): the BSDF layer as this family's TRACE unit compiled it, in every family's module ----
#if PPG_FAMILY == PPG_FAMILY_BASE
#define k_debug_bsdf k_debug_bsdf_base
#elif PPG_FAMILY != PPG_FAMILY_EXT
#define k_debug_bsdf PPG_FAMILY_NAME(k_debug_bsdf)  // (the ext family's is the unsuffixed one)
#endif
// unit FULL: the material as shade_one prepares it at a hit with texture coordinates uv, then the render's mat_eval / mat_pdf / mat_sample
__global__ void k_debug_bsdf(DevScene S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = debug_bsdf_full(S, items[i]);
}
#if PPG_FAMILY == PPG_FAMILY_BASE
// unit LEAN: the material as the !FULL branch of shade_one loads it — type, no flags, the reflectance — then bsdf_eval / bsdf_pdf /
// bsdf_sample; eta and the null flag are what shade_one keeps beside them (sampledEta = 1, sampledNull = false)
__global__ void k_debug_bsdf_lean(DevScene S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ppg_debug_bsdf_item it = items[i];
    const float4 mat = S.materials[PPG_MAT_STRIDE * (size_t)it.material];
    const int type = (int)mat.w;
    const F3 refl = f3(mat.x, mat.y, mat.z);
    const F3 wi = f3(it.wi[0], it.wi[1], it.wi[2]), wo = f3(it.wo[0], it.wo[1], it.wo[2]);
    ppg_debug_bsdf_out r;
    memset(&r, 0, sizeof r);
    const F3 f = bsdf_eval(type, refl, wi, wo);
    r.eval[0] = f.x; r.eval[1] = f.y; r.eval[2] = f.z;
    r.pdf = bsdf_pdf(type, wi, wo);
    F3 swo;
    float spdf;
    bool delta;
    const F3 w = bsdf_sample(type, refl, wi, it.sample[0], it.sample[1], swo, spdf, delta);
    r.wo[0] = swo.x; r.wo[1] = swo.y; r.wo[2] = swo.z;
    r.sampled_pdf = spdf;
    r.weight[0] = w.x; r.weight[1] = w.y; r.weight[2] = w.z;
    r.eta = 1.0f; r.delta = delta ? 1 : 0;
    r._pad[0] = debug_bsdf_flag_bits(bsdf_is_smooth(type), type == PPG_BSDF_TWOSIDED_DIFFUSE, false);
    out[i] = r;
}
#endif
static void launch_debug_bsdf(int lean, int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
#if PPG_FAMILY == PPG_FAMILY_BASE
    if (lean) { hipLaunchKernelGGL(k_debug_bsdf_lean, dim3(grid), dim3(block), 0, stream, S, n, items, out); return; }
#endif
    hipLaunchKernelGGL(k_debug_bsdf, dim3(grid), dim3(block), 0, stream, S, n, items, out);  // (the hook has refused LEAN elsewhere)
}

#if PPG_FAMILY == PPG_FAMILY_LOBES
// ppg_debug_shading_frame: the closest hit, then what shade_one does for the frame of a textured BSDF — fill_isect_tex, and bump_frame or
// normal_frame where the material's texture word names a displacement texture or a normal map
__global__ void k_debug_shading_frame(DevScene S, unsigned int n, const float4 *rays, ppg_debug_frame *out) {
    extern __shared__ int dbg_stack[];
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
    const F3 o = f3(ro.x, ro.y, ro.z), d = f3(rd.x, rd.y, rd.z);
    ppg_debug_frame r;
    memset(&r, 0, sizeof r);
    r.material = -1;
    const Hit h = trace_closest4<false, true>(S, dbg_stack + threadIdx.x, (int)blockDim.x, o, d, ro.w, rd.w);
    r.prim = h.prim;
    if (h.prim >= 0) {
        Isect I;
        TexInfo X;
        X.tex = 0u; X.u = 0.0f; X.v = 0.0f;
        if (h.prim >= S.n_tris) fill_isect_analytic(S, h, o, d, I);
        else fill_isect_tex<true>(S, h, d, I, X);
        F3 ps = I.s, pt = I.t, pn = I.n;
        if (X.tex >> 16) {
            const int flags = __float_as_int(S.materials[PPG_MAT_STRIDE * (size_t)I.material + 2].w);
            if (flags & PPG_MAT_NORMALMAP) normal_frame(S, I, X, ps, pt, pn);
            else bump_frame(S, I, X, ps, pt, pn);
            r.adapted = 1;
        }
        r.material = I.material;
        r.uv[0] = X.u; r.uv[1] = X.v;
        r.n[0] = I.n.x; r.n[1] = I.n.y; r.n[2] = I.n.z;
        r.s[0] = I.s.x; r.s[1] = I.s.y; r.s[2] = I.s.z;
        r.ps[0] = ps.x; r.ps[1] = ps.y; r.ps[2] = ps.z;
        r.pt[0] = pt.x; r.pt[1] = pt.y; r.pt[2] = pt.z;
        r.pn[0] = pn.x; r.pn[1] = pn.y; r.pn[2] = pn.z;
    }
    out[i] = r;
}
static void launch_debug_shading_frame(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_frame *out) {
    hipLaunchKernelGGL(k_debug_shading_frame, dim3(grid), dim3(block), (size_t)PPG_LDS_STACK * block * sizeof(int), stream, S, n, rays, out);
}
#endif

// ---- ppg_debug_sample_direct(_as) / ppg_debug_pdf_direct: the two halves of the direct-light MIS, in every family's module ----
#define k_debug_sample_direct PPG_FAMILY_NAME(k_debug_sample_direct)
#define k_debug_pdf_direct PPG_FAMILY_NAME(k_debug_pdf_direct)
// emitter_sample_direct<FULL> as this module compiled it; the record is the DirectSample as the function left it
template <bool FULL>
__global__ void k_debug_sample_direct(DevScene S, unsigned int n, const float *ref, const float *refN, const float *u, ppg_debug_direct_ex *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DirectSample ds;
    const F3 value = emitter_sample_direct<FULL>(S, f3(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]), f3(refN[3 * i], refN[3 * i + 1], refN[3 * i + 2]),
                                                 u[2 * i], u[2 * i + 1], ds);
    ppg_debug_direct_ex r;
    memset(&r, 0, sizeof r);
    const int n_sel = S.n_emitters + (FULL ? S.n_delta : 0) + (S.env.w != 0 ? 1 : 0);
    r.emitter = n_sel ? pmf_sample(S.em_sel_cdf, n_sel + 1, u[2 * i]) : -1;  // the choice emitter_sample_direct makes
    r.d[0] = ds.d.x; r.d[1] = ds.d.y; r.d[2] = ds.d.z; r.dist = ds.dist;
    r.n[0] = ds.n.x; r.n[1] = ds.n.y; r.n[2] = ds.n.z;
    r.pdf = ds.pdf; r.em_pdf = ds.em_pdf;
    r.value[0] = value.x; r.value[1] = value.y; r.value[2] = value.z;
    r.sd[0] = ds.sd.x; r.sd[1] = ds.sd.y; r.sd[2] = ds.sd.z; r.sdist = ds.sdist;
    r.is_env = ds.is_env ? 1 : 0; r.is_delta = ds.is_delta ? 1 : 0;
    out[i] = r;
}
// the FL_PENDING branch of shade_one (ppg_kernels.h) up to emitterPdf, for a ray that left a vertex whose DirectSamplingRecord normal is
// refN (0: none): closest hit, the FULL kernels' record, eval_Le or the environment emitter, then the render's own emitter_pdf_direct
__global__ void k_debug_pdf_direct(DevScene S, unsigned int n, const float4 *rays, const float *refN, ppg_debug_pdf *out) {
    extern __shared__ int dbg_stack[];
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
    const F3 o = f3(ro.x, ro.y, ro.z), d = f3(rd.x, rd.y, rd.z), rn = f3(refN[3 * i], refN[3 * i + 1], refN[3 * i + 2]);
    ppg_debug_pdf r;
    memset(&r, 0, sizeof r);
    const Hit h = trace_closest4<false, true>(S, dbg_stack + threadIdx.x, (int)blockDim.x, o, d, ro.w, rd.w);
    const bool valid = h.prim >= 0;
    Isect I;
    I.n = f3s(0.0f); I.emitter = -1;
    if (valid) fill_isect_full(S, h, o, d, I);
    F3 value = valid ? eval_Le(S, I, -d) : f3s(0.0f);
    const F3 em_n = I.n;
    const float em_dist = h.t;
    int em_id = I.emitter;
    if (!valid && S.env.w != 0 && env_fill_direct(S, o, d)) { value = env_radiance(S, d); em_id = S.n_emitters + S.n_delta; }
    const bool noRefN = rn.x == 0 && rn.y == 0 && rn.z == 0;
    const bool refn_ok = dot3(d, rn) >= 0;                    // FL_PEND_REFN as shade_one sets it when it samples the bounce
    const float nee_cos = noRefN ? -2.0f : dot3(d, rn);       // P.nee_cos likewise
    float pdfDirect = 0.0f;
    if (!iszero3(value)) pdfDirect = emitter_pdf_direct<true>(S, em_id, d, em_n, em_dist, refn_ok, [&]() { return nee_cos; }, [&]() { return ro; });
    r.prim = h.prim; r.emitter = em_id;
    r.value[0] = value.x; r.value[1] = value.y; r.value[2] = value.z;
    r.pdf_direct = pdfDirect;
    r.emitter_pdf = pdfDirect * (1.0f * S.em_sel_norm);
    out[i] = r;
}
static void launch_debug_sample_direct(int full, int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float *ref, const float *ref_n,
                                       const float *u, ppg_debug_direct_ex *out) {
#if PPG_FAMILY == PPG_FAMILY_BASE
    if (!full) { hipLaunchKernelGGL((k_debug_sample_direct<false>), dim3(grid), dim3(block), 0, stream, S, n, ref, ref_n, u, out); return; }
#endif
    hipLaunchKernelGGL((k_debug_sample_direct<true>), dim3(grid), dim3(block), 0, stream, S, n, ref, ref_n, u, out);  // (the hook has refused full = 0 elsewhere)
}
static void launch_debug_pdf_direct(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, const float *ref_n, ppg_debug_pdf *out) {
    hipLaunchKernelGGL(k_debug_pdf_direct, dim3(grid), dim3(block), (size_t)PPG_LDS_STACK * block * sizeof(int), stream, S, n, rays, ref_n, out);
}

// ---- ppg_debug_math_eval / ppg_debug_math_checksum: include/ppg_mathcheck.h on the device, in every family's module ----
#define k_debug_math_eval PPG_FAMILY_NAME(k_debug_math_eval)
#define k_debug_math_checksum PPG_FAMILY_NAME(k_debug_math_checksum)
// VIA = 0: the header's functions, inlined here.  VIA = 1: what the kernels of this module call — its out-of-line dm_sincos, dm_atan2, dm_exp,
// dm_log and the dm_acos, dm_tan, dm_pow built on them (ppg_device.h); only for the ops of ppg_mathcheck_has_dm.
template <int VIA> D void debug_math_eval(int op, uint32_t a, uint32_t b, uint32_t *o0, uint32_t *o1) {
    if (VIA == 0) { ppg_mathcheck_eval(op, a, b, o0, o1); return; }
    const float fa = ppg_u2f(a), fb = ppg_u2f(b);
    switch (op) {
        case 0: { const float2 r = dm_sincos(fa); *o0 = ppg_f2u(r.x); *o1 = ppg_f2u(r.y); break; }
        case 1: *o0 = ppg_f2u(dm_atan2(fa, fb)); break;
        case 2: *o0 = ppg_f2u(dm_exp(fa)); break;
        case 6: *o0 = ppg_f2u(dm_log(fa)); break;
        case 7: *o0 = ppg_f2u(dm_pow(fa, fb)); break;
        case 11: *o0 = ppg_f2u(dm_acos(fa)); break;
        case 12: *o0 = ppg_f2u(dm_tan(fa)); break;
        default: break;  // (the hook has refused the op)
    }
}
template <int VIA> __global__ void k_debug_math_eval(int op, unsigned int n, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ua = ppg_mathcheck_arg_a(op, i, a[i]), ub = b[i];
    if (!ppg_mathcheck_in_domain(op, ua, ub)) return;  // (its outputs stay as the host sent them)
    uint32_t o0 = 0u, o1 = 0u;
    debug_math_eval<VIA>(op, ua, ub, &o0, &o1);
    out0[i] = o0;
    if (ppg_mathcheck_outputs(op) == 2) out1[i] = o1;
}
// PPG_MATH_GROUPS workgroups of 256 share a block of 2^24 patterns: slot = blockIdx.x / PPG_MATH_GROUPS < n_blocks by the size of the grid.
// Each lane sums the terms of its stride, a wave adds its lanes' sums by shuffles, its first lane adds the wave's to the block's slot.
#define PPG_MATH_GROUPS 64u
template <int VIA> __global__ __launch_bounds__(256) void k_debug_math_checksum(int op, unsigned int first_block, unsigned int n_blocks, unsigned long long *out) {
    const unsigned int slot = blockIdx.x / PPG_MATH_GROUPS;
    if (slot >= n_blocks) return;
    const uint32_t base = (first_block + slot) << PPG_MATHCHECK_BLOCK_BITS;
    const unsigned int stride = PPG_MATH_GROUPS * 256u;
    const int nf = ppg_mathcheck_float_outputs(op);
    unsigned long long sum = 0ull;
    for (unsigned int i = (blockIdx.x % PPG_MATH_GROUPS) * 256u + threadIdx.x; i < (1u << PPG_MATHCHECK_BLOCK_BITS); i += stride) {
        const uint32_t u = base | i;
        if (!ppg_mathcheck_in_domain(op, u, 0u)) continue;
        uint32_t o0 = 0u, o1 = 0u;
        debug_math_eval<VIA>(op, u, 0u, &o0, &o1);
        if (nf > 0) o0 = ppg_mathcheck_canon(o0);
        if (nf > 1) o1 = ppg_mathcheck_canon(o1);
        sum += ppg_mathcheck_mix(u, o0, o1);
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned int lo = __shfl_down((unsigned int)sum, d, 64), hi = __shfl_down((unsigned int)(sum >> 32), d, 64);
        sum += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63u) == 0u) atomicAdd(out + slot, sum);
}
static void launch_debug_math_eval(hipStream_t stream, int via, int op, unsigned int n, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1) {
    const dim3 grid((n + 255u) / 256u), block(256);
    if (via) hipLaunchKernelGGL((k_debug_math_eval<1>), grid, block, 0, stream, op, n, a, b, out0, out1);
    else hipLaunchKernelGGL((k_debug_math_eval<0>), grid, block, 0, stream, op, n, a, b, out0, out1);
}
static void launch_debug_math_checksum(hipStream_t stream, int via, int op, unsigned int first_block, unsigned int n_blocks, unsigned long long *out) {
    const dim3 grid(n_blocks * PPG_MATH_GROUPS), block(256);
    if (via) hipLaunchKernelGGL((k_debug_math_checksum<1>), grid, block, 0, stream, op, first_block, n_blocks, out);
    else hipLaunchKernelGGL((k_debug_math_checksum<0>), grid, block, 0, stream, op, first_block, n_blocks, out);
}

#if PPG_FAMILY == PPG_FAMILY_MEDIA
// ppg_debug_medium: medium_sample_distance, medium_transmittance, phase_sample and phase_eval as this family's kernels compile them, item by
// item.  The ray starts at the origin and runs along -wi; u[0], u[1] feed sampleDistance (u[1] only where it draws a second number),
// u[2], u[3] the phase sample.
__global__ void k_debug_medium(MediaArgs M, unsigned int n, const ppg_debug_medium_item *items, ppg_debug_medium_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ppg_debug_medium_item it = items[i];
    const float4 *Q = medium_record(M.media, (unsigned int)it.medium + 1u);
    const F3 wi = f3(it.wi[0], it.wi[1], it.wi[2]);
    ppg_debug_medium_out r;
    memset(&r, 0, sizeof r);
    MediumSample ms;
    int drawn = 0;
    r.success = medium_sample_distance(Q, f3s(0.0f), -wi, it.length, [&]() { return it.u[drawn++ ? 1 : 0]; }, ms) ? 1 : 0;
    r.t = ms.t; r.pdf_success = ms.pdfSuccess; r.pdf_failure = ms.pdfFailure;
    r.transmittance[0] = ms.transmittance.x; r.transmittance[1] = ms.transmittance.y; r.transmittance[2] = ms.transmittance.z;
    const F3 tr = medium_transmittance(Q, it.length);
    r.eval_transmittance[0] = tr.x; r.eval_transmittance[1] = tr.y; r.eval_transmittance[2] = tr.z;
    F3 wo;
    r.phase_pdf = phase_sample(Q, wi, it.u[2], it.u[3], wo);
    r.wo[0] = wo.x; r.wo[1] = wo.y; r.wo[2] = wo.z;
    r.phase_eval = phase_eval(Q, wi, wo);
    out[i] = r;
}
static void launch_debug_medium(int grid, int block, hipStream_t stream, const MediaArgs &M, unsigned int n, const ppg_debug_medium_item *items, ppg_debug_medium_out *out) {
    hipLaunchKernelGGL(k_debug_medium, dim3(grid), dim3(block), 0, stream, M, n, items, out);
}
#endif

#if PPG_FAMILY == PPG_FAMILY_HETMEDIA
// ppg_debug_volume: volume_lookup_float / volume_lookup_rgb as this family's kernels compile them, item by item (the host has checked
// every index)
__global__ void k_debug_volume(HetArgs V, unsigned int n, const ppg_debug_volume_item *items, ppg_debug_volume_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ppg_debug_volume_item it = items[i];
    const F3 p = f3(it.p[0], it.p[1], it.p[2]);
    ppg_debug_volume_out r;
    const int channels = __float_as_int(V.volumes[PPG_VOLUME_STRIDE * (size_t)it.volume].x) >> 8;
    if (channels == 1) { r.value[0] = volume_lookup_float(V.volumes, V.pool, it.volume, p); r.value[1] = r.value[2] = 0.0f; }
    else { const F3 v = volume_lookup_rgb(V.volumes, V.pool, it.volume, p); r.value[0] = v.x; r.value[1] = v.y; r.value[2] = v.z; }
    out[i] = r;
}
static void launch_debug_volume(int grid, int block, hipStream_t stream, const HetArgs &V, unsigned int n, const ppg_debug_volume_item *items, ppg_debug_volume_out *out) {
    hipLaunchKernelGGL(k_debug_volume, dim3(grid), dim3(block), 0, stream, V, n, items, out);
}
// ppg_debug_hetmedium: hetmedium_sample_distance on the ray over [0, maxt], then hetmedium_transmittance on the same ray, the random
// numbers ppg_rand(key, dim), ppg_rand(key, dim + 1), .. in that order
__global__ void k_debug_hetmedium(HetArgs V, unsigned int n, const ppg_debug_hetmedium_item *items, ppg_debug_hetmedium_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ppg_debug_hetmedium_item it = items[i];
    const float4 *Hr = het_record(V.het, (unsigned int)it.medium + 1u);
    const F3 o = f3(it.o[0], it.o[1], it.o[2]), d = f3(it.d[0], it.d[1], it.d[2]);
    unsigned int dim = it.dim;
    const unsigned int key = it.key;
    ppg_debug_hetmedium_out r;
    HetSample hs;
    r.success = hetmedium_sample_distance(V.volumes, V.pool, Hr, o, d, 0.0f, it.maxt, [&]() { return ppg_rand(key, dim++); }, hs) ? 1 : 0;
    r.t = hs.t; r.sigma_s[0] = hs.sigmaS.x; r.sigma_s[1] = hs.sigmaS.y; r.sigma_s[2] = hs.sigmaS.z; r.transmittance = hs.transmittance;
    r.draws = dim - it.dim;
    const unsigned int dim1 = dim;
    r.eval_transmittance = hetmedium_transmittance(V.volumes, V.pool, Hr, o, d, 0.0f, it.maxt, [&]() { return ppg_rand(key, dim++); });
    r.eval_draws = dim - dim1;
    out[i] = r;
}
static void launch_debug_hetmedium(int grid, int block, hipStream_t stream, const HetArgs &V, unsigned int n, const ppg_debug_hetmedium_item *items, ppg_debug_hetmedium_out *out) {
    hipLaunchKernelGGL(k_debug_hetmedium, dim3(grid), dim3(block), 0, stream, V, n, items, out);
}
#endif

// the hooks' launchers of this family, into its row
static void fill_debug_kernels(PathKernels &K) {
    K.debug_math_eval = launch_debug_math_eval;
    K.debug_math_checksum = launch_debug_math_checksum;
    K.debug_sample_direct = launch_debug_sample_direct;
    K.debug_pdf_direct = launch_debug_pdf_direct;
#if PPG_FAMILY == PPG_FAMILY_SHAPES
    K.debug_intersect = launch_debug_intersect;
    K.debug_trace = launch_debug_trace;
    K.debug_hit_records = launch_debug_hit_records;
#endif
    K.debug_bsdf = launch_debug_bsdf;
#if PPG_FAMILY == PPG_FAMILY_LOBES
    K.debug_shading_frame = launch_debug_shading_frame;
#endif
#if PPG_FAMILY == PPG_FAMILY_MEDIA
    K.debug_medium = launch_debug_medium;
#endif
#if PPG_FAMILY == PPG_FAMILY_HETMEDIA
    K.debug_volume = launch_debug_volume;
    K.debug_hetmedium = launch_debug_hetmedium;
#endif
}

#endif
