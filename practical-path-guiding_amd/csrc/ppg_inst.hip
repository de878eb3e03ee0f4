/*
 * ppg_inst.hip — the large path kernels, a few instantiations per translation unit (ppg_launch.h).  A unit is compiled for a kernel family,
 * -DPPG_FAMILY=f (ppg_device.h), and for one role in it:
 *   -DPPG_UNIT_SHADE         k_shade<NEE, FULL>           -DPPG_UNIT_TAIL          k_tail<SMALL, NEE, FULL>
 *   -DPPG_UNIT_TRACE         k_trace<SMALL, COUNT>, the kernels of the test hooks that belong to the family (ppg_debug_kernels.h) and, in the
 *                            top family, those of ppg_render_fields (ppg_fields_kernels.h)
 * A family above the base is three such units: its scenes are FULL and never SMALL.  The base family splits the first two further, one
 * -DPPG_UNIT_PART=p per unit (k_shade: p = NEE; k_tail: p = SMALL * 2 + NEE; both FULL settings each), and has two units outside the families:
 *   -DPPG_UNIT_SHADE_COMMON  k_shade<false, true, MSET_COMMON>: the common material classes of a FULL scene; k_debug_bsdf_common, the
 *                            test hook's kernel over this unit's copy of the BSDF layer (ppg_debug_bsdf.h)
 *   -DPPG_UNIT_COMMIT        k_commit (all six), k_commit_records and k_splat_sorted
 * The unit enters its launchers into its family's row of ppg_path_kernels when the library is loaded.
 */
#include <hip/hip_runtime.h>

#ifdef PPG_UNIT_SHADE_COMMON
#define PPG_PARAM_TEXTURES 0  // k_shade<.., MSET_COMMON> reads no bitmap on specular / alpha / opacity (ppg_device.h mat_spec_lum)
#endif
#include "ppg_launch.h"

#define PPG_BASE_ONLY (PPG_FAMILY == PPG_FAMILY_BASE)  // the kernels without the FULL material set, and those of SMALL scenes
#define ROW ppg_path_kernels[PPG_FAMILY]               // this unit's family's
#define PPG_FILL_ROW __attribute__((constructor)) static void fill_row()
// the media family's kernels take the scene and the path state with MediaArgs appended (ppg_device.h SceneArg, ppg_kernels.h PathArg)
// (and the hetmedia family's with HetArgs on top of that)
#if PPG_MEDIA
static PathArg path_arg(const PathState &P, const MediaArgs &M) { PathArg r; static_cast<PathState &>(r) = P; r.medium = {M.path_medium, M.path_stride}; return r; }
#else
static const PathState &path_arg(const PathState &P, const MediaArgs &) { return P; }
#endif
#if PPG_HETMEDIA
static SceneArg scene_arg(const DevScene &S, const MediaArgs &M, const HetArgs &V) {
    SceneArg r; static_cast<DevScene &>(r) = S; r.media = M.media; r.prim_media = M.prim_media; r.volumes = V.volumes; r.pool = V.pool; r.het = V.het; return r;
}
#elif PPG_MEDIA
static SceneArg scene_arg(const DevScene &S, const MediaArgs &M, const HetArgs &) { SceneArg r; static_cast<DevScene &>(r) = S; r.media = M.media; r.prim_media = M.prim_media; return r; }
#else
static const DevScene &scene_arg(const DevScene &S, const MediaArgs &, const HetArgs &) { return S; }
#endif

#if defined(PPG_UNIT_SHADE)
template <bool NEE, bool FULL> static void launch_shade(const ShadeLaunch &a) {
    hipLaunchKernelGGL((k_shade<NEE, FULL>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, path_arg(a.P, a.M), scene_arg(a.S, a.M, a.V), a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
}
template <bool NEE> static void shade(int variant, const ShadeLaunch &a) {
#if PPG_BASE_ONLY
    if (!(variant & 1)) { launch_shade<NEE, false>(a); return; }
#endif
    launch_shade<NEE, true>(a);
}
PPG_FILL_ROW {
#ifdef PPG_UNIT_PART
    ROW.shade[PPG_UNIT_PART] = shade<PPG_UNIT_PART != 0>;
#else
    ROW.shade[0] = shade<false>;
    ROW.shade[1] = shade<true>;
#endif
}
#elif defined(PPG_UNIT_TAIL)
template <bool SMALL, bool NEE, bool FULL> static void launch_tail(const TailLaunch &a) {
    hipLaunchKernelGGL((k_tail<SMALL, NEE, FULL>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, path_arg(a.P, a.M), scene_arg(a.S, a.M, a.V), a.T, a.R, a.dense, a.total, a.ticket, a.stats, a.lds_tris, a.longest, a.strag, a.lane_limit);
}
template <bool SMALL, bool NEE> static void tail(int variant, const TailLaunch &a) {
#if PPG_BASE_ONLY
    if (!(variant & 1)) { launch_tail<SMALL, NEE, false>(a); return; }
#endif
    launch_tail<SMALL, NEE, true>(a);
}
PPG_FILL_ROW {
#ifdef PPG_UNIT_PART
    ROW.tail[PPG_UNIT_PART] = tail<(PPG_UNIT_PART & 2) != 0, (PPG_UNIT_PART & 1) != 0>;
#else
    ROW.tail[0] = tail<false, false>;
    ROW.tail[1] = tail<false, true>;
#endif
}
#elif defined(PPG_UNIT_TRACE)
#include "ppg_debug_kernels.h"
#include "ppg_fields_kernels.h"
template <bool SMALL, bool COUNT> static void launch_trace(const TraceLaunch &a) {
    hipLaunchKernelGGL((k_trace<SMALL, COUNT>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.Q, a.qin, a.lds_nodes, a.lds_tris, a.sorted, a.keys);
}
static void trace(const TraceLaunch &a) {
#if PPG_BASE_ONLY
    if (a.small) { launch_trace<true, false>(a); return; }
#endif
    if (a.count) launch_trace<false, true>(a);
    else launch_trace<false, false>(a);
}
PPG_FILL_ROW {
    ROW.trace = trace;
    fill_debug_kernels(ROW);
    fill_fields_kernels(ROW);
}
#elif defined(PPG_UNIT_SHADE_COMMON)
#include "ppg_debug_bsdf.h"
void ppg_launch_shade_common(const ShadeLaunch &a) {
    hipLaunchKernelGGL((k_shade<false, true, MSET_COMMON>), dim3(a.grid), dim3(PPG_BLOCK), a.lds, a.stream, a.P, a.S, a.T, a.R, a.Q, a.qin, a.small_scene, a.sorted_items);
}
// ppg_debug_bsdf_as, unit COMMON: this unit's mat_eval / mat_pdf / mat_sample, item by item (the host has refused what sort_slice keeps out
// of the common part)
__global__ void k_debug_bsdf_common(DevScene S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = debug_bsdf_full(S, items[i]);
}
void ppg_launch_debug_bsdf_common(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    hipLaunchKernelGGL(k_debug_bsdf_common, dim3(grid), dim3(block), 0, stream, S, n, items, out);
}
#elif defined(PPG_UNIT_COMMIT)
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
#else
#error "compile with -DPPG_FAMILY=f and one of -DPPG_UNIT_SHADE, _TAIL, _TRACE, _SHADE_COMMON, _COMMIT"
#endif
