/*
 * ppg_launch.h — launchers of the large path kernels.  In the base family k_shade exists in five instantiations (NEE x FULL, and MSET_COMMON),
 * k_tail in eight (SMALL x NEE x FULL), k_trace in three and k_commit in six (spatial x directional filter); every further family
 * (ppg_device.h PPG_FAMILY) adds the FULL ones of k_shade, k_tail and k_trace.  Each pair of instantiations is its own translation unit
 * (ppg_inst.hip compiled for a family and a role), so the library builds in parallel instead of in one 2.5-minute compile.  No device code
 * crosses a translation unit: a unit hands the host a launcher — an argument struct per role, a table of launchers per family.
 */
#ifndef PPG_LAUNCH_H
#define PPG_LAUNCH_H

#include "ppg_kernels.h"

struct ShadeLaunch {
    int grid;
    size_t lds;
    hipStream_t stream;
    PathState P; DevScene S; DevTree T; RenderParams R; Queues Q;
    int qin, small_scene;
    const unsigned int *sorted_items;
    MediaArgs M;             // the media family's extra arguments (ppg_device.h); zero: the scene binds no medium
    HetArgs V;               // the hetmedia family's, on top of M; zero: no bound medium is heterogeneous
};
struct TailLaunch {
    int grid;
    size_t lds;
    hipStream_t stream;
    PathState P; DevScene S; DevTree T; RenderParams R;
    const unsigned int *dense;
    const unsigned long long *total;
    unsigned int *ticket;
    BlockStats *stats;
    int lds_tris;
    unsigned int *longest;   // the longest path (bounces) this launch finishes: what its duration is made of
    StragOut strag;          // R.defer_depth > 0: where the paths still alive at that depth go
    unsigned int lane_limit; // paths a wave takes at a time (64; fewer for a launch over a handful of stragglers)
    MediaArgs M;             // the media family's extra arguments (ppg_device.h); zero: the scene binds no medium
    HetArgs V;               // the hetmedia family's, on top of M; zero: no bound medium is heterogeneous
};
struct TraceLaunch {
    int grid;
    size_t lds;
    hipStream_t stream;
    PathState P; DevScene S; Queues Q;
    int qin, lds_nodes, lds_tris;
    unsigned int *sorted;    // sort_slice's output and key scratch; null: the slices are not sorted
    unsigned char *keys;
    bool small;              // the scene is traced from LDS (k_trace<true>: base family only)
    bool count;              // count the BVH nodes and triangles visited (kernel timing)
};
struct CommitLaunch {
    int grid;
    hipStream_t stream;
    PathState P; DevTree T; RenderParams R; Queues Q;
    const unsigned char *nv8;   // k_commit_prepare's byte per path, k_commit_prepare_list's per list entry
    const unsigned int *list;
    const unsigned long long *list_n;
    float4 *splat;              // k_commit_records: the round's splat records
    unsigned int flag_shift;    // ... and the key bit of "a splat only"
};
struct SplatLaunch {
    int grid;
    hipStream_t stream;
    DevTree T;
    const unsigned long long *keys;
    const unsigned int *idx;
    const float4 *splat;
    unsigned int n, leaf_bits;
    unsigned int lds_nodes;     // D-trees of up to this many nodes are staged in LDS (<= PPG_SPLAT_NODES)
};

// ppg_render_fields (ppg_fields_kernels.h): one sample pass of the whole film, then its resolve pass
struct FieldsRequest {
    int n_fields;
    int field[PPG_MAX_FIELDS];          // PPG_FIELD_*
    float undefined[PPG_MAX_FIELDS][3];
    int albedo;                         // PPG_FIELD_ALBEDO is among them: the hit's material and its bitmaps are read
    float w2c[16];                      // the inverse of the camera's camera_to_world (REL_POSITION)
};
struct FieldsSampleLaunch {
    hipStream_t stream;
    DevScene S;
    FieldsRequest F;
    unsigned long long seed;
    unsigned int sample;                // the sample index of this pass
    const float *albedo_scale;          // per material: what multiplies the diffuse reflectance (0: no diffuse reflection)
    float *vals;                        // [n_fields][3][W * H]: the sample's value per field, channel and pixel
    float *pos;                         // [2][W * H]: its film position - 0.5 (ImageBlock::put)
};
struct FieldsResolveLaunch {
    hipStream_t stream;
    FilmFilter ff;
    int border, n_fields;
    const float *vals, *pos;
    float *sum;                         // [n_fields][W * H][3]
    float *wsum;                        // [W * H]
};

// One row per kernel family (ppg_device.h PPG_FAMILY): the launchers of its k_shade, k_tail and k_trace.  Every unit of ppg_inst.hip enters the
// launchers it defines into its family's row when the library is loaded; the host picks the row with sceneFamily (ppg_hip.hip).
struct ppg_debug_hit;
struct ppg_debug_direct_ex;
struct ppg_debug_pdf;
struct ppg_debug_bsdf_item;
struct ppg_debug_bsdf_out;
struct ppg_debug_frame;
struct ppg_debug_medium_item;
struct ppg_debug_medium_out;
struct ppg_debug_volume_item;
struct ppg_debug_volume_out;
struct ppg_debug_hetmedium_item;
struct ppg_debug_hetmedium_out;
struct PathKernels {
    void (*shade[2])(int variant, const ShadeLaunch &a);  // [NEE]; variant = (NEE ? 2 : 0) | (FULL ? 1 : 0)
    void (*tail[4])(int variant, const TailLaunch &a);    // [SMALL * 2 + NEE]; variant = (SMALL ? 4 : 0) | (NEE ? 2 : 0) | (FULL ? 1 : 0)
    void (*trace)(const TraceLaunch &a);
    // The kernels of the test hooks (ppg_debug_kernels.h), in the families that compile them: the shapes family those of ppg_debug_intersect,
    // the top family that of ppg_debug_shading_frame
    void (*debug_intersect)(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_hit *out, int any);
    void (*debug_trace)(int mode, int param, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_hit *out, unsigned int *stats);
    void (*debug_hit_records)(hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, const float4 *hits, ppg_debug_hit *out);
    void (*debug_shading_frame)(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, ppg_debug_frame *out);
    // the top family: the kernels of ppg_render_fields (ppg_fields_kernels.h), which know every material and shape a scene may hold
    void (*fields_sample)(const FieldsSampleLaunch &a);
    void (*fields_resolve)(const FieldsResolveLaunch &a);
    // every family: include/ppg_mathcheck.h as the family's TRACE unit compiled it (via = 1: through the unit's dm_ copies)
    void (*debug_math_eval)(hipStream_t stream, int via, int op, unsigned int n, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1);
    void (*debug_math_checksum)(hipStream_t stream, int via, int op, unsigned int first_block, unsigned int n_blocks, unsigned long long *out);
    // every family: its copy of emitter_sample_direct<full != 0> (full = 0: the base family only) and of the pending bounce's emitter density
    void (*debug_sample_direct)(int full, int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float *ref, const float *ref_n,
                                const float *u, ppg_debug_direct_ex *out);
    void (*debug_pdf_direct)(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const float4 *rays, const float *ref_n, ppg_debug_pdf *out);
    // every family: its copy of mat_eval / mat_pdf / mat_sample (lean != 0: bsdf_eval / bsdf_pdf / bsdf_sample, the base family only)
    void (*debug_bsdf)(int lean, int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out);
    // the media family: its medium_sample_distance / medium_transmittance / phase_sample / phase_eval (ppg_debug_medium)
    void (*debug_medium)(int grid, int block, hipStream_t stream, const MediaArgs &M, unsigned int n, const ppg_debug_medium_item *items, ppg_debug_medium_out *out);
    // the hetmedia family: its volume lookups (ppg_debug_volume) and its tracking routines (ppg_debug_hetmedium)
    void (*debug_volume)(int grid, int block, hipStream_t stream, const HetArgs &V, unsigned int n, const ppg_debug_volume_item *items, ppg_debug_volume_out *out);
    void (*debug_hetmedium)(int grid, int block, hipStream_t stream, const HetArgs &V, unsigned int n, const ppg_debug_hetmedium_item *items, ppg_debug_hetmedium_out *out);
};
extern PathKernels ppg_path_kernels[PPG_FAMILIES];

// The kernels outside the families, each defined in the unit that compiles it.
// k_shade<false, FULL, MSET_COMMON> over the front part of the sorted slices (a.qin = QIN_SORTED_COMMON)
void ppg_launch_shade_common(const ShadeLaunch &a);
// ppg_debug_bsdf_as, unit COMMON: mat_eval / mat_pdf / mat_sample as that unit compiled them (PPG_PARAM_TEXTURES = 0)
void ppg_launch_debug_bsdf_common(int grid, int block, hipStream_t stream, const DevScene &S, unsigned int n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out);
void ppg_launch_commit(int spatial_filter, int directional_filter, const CommitLaunch &a);
// a round of the optimiser: k_commit_records (nearest / stochastic spatial filter), then — after the sort — k_splat_sorted
void ppg_launch_commit_records(int spatial_filter, const CommitLaunch &a);
void ppg_launch_splat(int directional_filter, const SplatLaunch &a);

#endif
