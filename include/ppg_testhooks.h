/*
 * ppg_testhooks.h — entry points of libppg_hip.so that exist for the tests only.  Not part of the drop-in boundary (include/ppg.h): nothing
 * a host of the integrator needs, no reference counterpart.
 *   host only   ppg_debug_build_bvh, ppg_debug_bvh_stats, ppg_debug_bvh_trace, ppg_debug_rfilter_table, ppg_debug_stree_depth
 *   a scene     ppg_debug_intersect, ppg_debug_intersect_mode, ppg_debug_sample_direct, ppg_debug_sample_direct_as, ppg_debug_pdf_direct,
 *               ppg_debug_bsdf, ppg_debug_bsdf_as, ppg_debug_shading_frame, ppg_debug_camera_rays
 *   a render    ppg_debug_set_defer_depth, ppg_debug_commit (inside an open training iteration)
 *   no scene    ppg_debug_math_eval, ppg_debug_math_checksum
 */
#ifndef PPG_TESTHOOKS_H
#define PPG_TESTHOOKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only (no GPU is touched): the quantised 4-wide BVH that ppg_set_scene builds for the traversal kernels, from a triangle
   soup.  nodes_out receives up to nodes_cap 64-byte nodes — { float origin[3]; uint32 exps (byte a = biased exponent of the power-of-two cell
   size along axis a); uint32 qlo[3] (x, y, z: child k's lower plane in byte k); uint32 qhi[3]; int32 child[4] (>= 0 node, < 0 leaf:
   ~child = first << 3 | count - 1 in leaf order, 0x7fffffff unused); int32 pad[2] } —, *n_nodes their number (also when it exceeds the
   capacity), order_out[n_triangles] the triangles in leaf order.  tests/test_bvh_host.py checks with it, on the CPU, that no child box on
   the way to a triangle a ray hits is ever missed under the kernels' float arithmetic (csrc/ppg_device.h bvh4_children). */
int ppg_debug_build_bvh(const float *positions, const uint32_t *indices, uint32_t n_triangles, float pad_abs, int32_t max_leaf,
                        void *nodes_out, uint32_t nodes_cap, uint32_t *n_nodes, uint32_t *order_out);

/* Host only: the quality of the tree ppg_debug_build_bvh returns, measured on the finished QUANTISED nodes with every child box decoded
   as the kernels decode it (origin + byte * cell).  sa_* are the expected-step figures of the surface area heuristic for a ray that
   enters the root's box: sa_interior = sum of area(child box) / area(root) over interior children (node steps below the root's own),
   sa_leaf the same over leaf children (leaf visits), sa_tris = sum of area / area(root) * triangles over leaf children (triangle tests).
   depth = 4-wide levels on the longest path; build_seconds = wall time of the builder alone.  stack_need = the most entries the ordered
   walk can leave on its stack: the maximum, over the paths from the root to a node, of the sum of (non-empty children - 1) over the
   interior nodes on the path.  The kernels' stacks hold 48 and ppg_set_scene hands them no tree that needs more. */
struct ppg_bvh_stats {
    uint32_t n_nodes, n_leaves, depth, n_binary_nodes;
    uint32_t leaf_hist[9]; /* [k] = leaves of k triangles */
    uint32_t stack_need;
    double sa_interior, sa_leaf, sa_tris;
    double build_seconds;
};
int ppg_debug_bvh_stats(const float *positions, const uint32_t *indices, uint32_t n_triangles, float pad_abs, int32_t max_leaf,
                        struct ppg_bvh_stats *out);

/* Host only: ordered closest-hit traversal of that tree on the CPU, in the kernels' float arithmetic (csrc/ppg_device.h bvh4_children,
   tri_hit_regs, trace_slice_bvh4: nearest child first, the others pushed farthest first, every test culled against the best hit so far,
   ties by original index).  rays = n_rays x { ox, oy, oz, mint, dx, dy, dz, maxt } (mint is taken as it stands).  Per ray: t_out (+inf
   without a hit), orig_out (original triangle index, -1 without), steps_out (node steps), tests_out (triangle tests); any may be NULL.
   *max_stack (may be NULL) receives the deepest traversal stack of all rays (the kernels' holds 48 entries). */
int ppg_debug_bvh_trace(const float *positions, const uint32_t *indices, uint32_t n_triangles, float pad_abs, int32_t max_leaf,
                        const float *rays, uint32_t n_rays, float *t_out, int32_t *orig_out, uint32_t *steps_out, uint32_t *tests_out,
                        uint32_t *max_stack);

/* Host only (no GPU is touched): the discretised filter ppg_set_rfilter would use — table[32] = ReconstructionFilter::m_values (31
   normalised samples and a 0), *radius = m_radius, *border = m_borderSize (rfilter.cpp:37-55).  Returns what ppg_set_rfilter would for
   the filter's own checks (PPG_ERR_INVALID for bad parameters or a border above 3). */
struct ppg_rfilter;
int ppg_debug_rfilter_table(const struct ppg_rfilter *f, float table[32], float *radius, int32_t *border);

/* The depth beyond which a path is a STRAGGLER (include/ppg.h: PPG_ADAM_DEFER_DEPTH = 64, part of the result).  One path in 10^4 gets there
   in a real scene and none in most test scenes; the parity tests lower it (1 .. 64; the oracle has the same switch, ppgo_debug_set_defer_depth)
   so that thousands of paths go through the stragglers' machinery — hand-over inside k_tail, the second launch beside the next round, the
   records applied one round late — and must still come out bit-equal to the oracle. */
struct ppg_ctx;
int ppg_debug_set_defer_depth(struct ppg_ctx *ctx, int32_t depth);

/* The traversal and the intersection record of the context's scene (after ppg_set_scene, outside a render), ray by ray: one small kernel
   whose lanes call what the render calls — trace_closest4 with the analytic passes behind it and the FULL kernels' intersection record
   (csrc/ppg_device.h).  rays = n x { ox, oy, oz, mint, dx, dy, dz, maxt }, mint as it stands.  prim: -1 = no hit; below the number of
   triangles a triangle (in the BVH's leaf order), then the spheres, then the shapes of ppg_set_shapes in their order.  any_hit != 0 runs
   the shadow rays' any-hit trace instead: only prim >= 0 (and, for an analytic hit, t) is meaningful then and no record is filled. */
struct ppg_debug_hit {
    int32_t prim;
    float t;
    float p[3], geo_n[3], n[3], s[3], wi[3];
    int32_t material, emitter;
    int32_t _pad;
};  /* 80 bytes */
int ppg_debug_intersect(struct ppg_ctx *ctx, uint32_t n, const float *rays, struct ppg_debug_hit *out, int32_t any_hit);

/* The shading frame a textured BSDF is queried in, ray by ray (rays as for ppg_debug_intersect, closest hit): one small kernel of the top
   kernel family whose lanes call what the render's shade_one calls — fill_isect_tex, then bump_frame (bumpmap.cpp:135-160) or normal_frame
   (normalmap.cpp:108-124) where bits 16..31 of the material's texture word are set.  prim as above (-1: no hit, material = -1, the rest 0);
   uv = its.uv (0 on a material that reads no bitmap, and on analytic shapes); n, s = the unperturbed shading frame's normal and tangent;
   ps, pt, pn = the frame the nested BSDF is queried in (= s, t, n where no adapter ran); adapted = 1 where one ran. */
struct ppg_debug_frame {
    int32_t prim, material;
    float uv[2];
    float n[3], s[3];
    float ps[3], pt[3], pn[3];
    int32_t adapted;
};  /* 80 bytes */
int ppg_debug_shading_frame(struct ppg_ctx *ctx, uint32_t n, const float *rays, struct ppg_debug_frame *out);

/* The camera rays of the context's scene (after ppg_set_scene, outside a render): the function k_generate and ppg_render_fields make a
   sample's ray with (csrc/ppg_device.h camera_ray), over the WHOLE film (a shard does not enter) for the sample indices first_sample ..
   first_sample + n_samples - 1 under the configured seed.  rays[(j * n_pixels + p) * 8 ..] = { ox, oy, oz, mint, dx, dy, dz, maxt } of
   pixel p (row-major), sample first_sample + j: the layout ppg_debug_intersect takes. */
int ppg_debug_camera_rays(struct ppg_ctx *ctx, uint32_t first_sample, uint32_t n_samples, float *rays /* [n_samples][n_pixels][8] */);

/* The same rays through the OTHER forms of the closest-hit traversal, each of which promises the same hit bit for bit (csrc/ppg_device.h,
   csrc/ppg_kernels.h); rays and records as above, mint as it stands except where noted.  stats_out (4 words, may be NULL) is zeroed, then:
     LANE, LANE_ANY, LANE_VOTE  trace_closest4<false | true, true, false | true>, one ray per lane in waves of 64 (LANE and LANE_ANY are what
                ppg_debug_intersect runs; VOTE, the leaf vote of k_tail's traversals, wants n to be a multiple of 64: whole waves).
     RESUME     trace_closest4_resume as k_tail's crowd phase drives it: a wave owns 512 consecutive rays; a lane that returned takes the
                wave's next ray, a lane that was parked calls again with resume = true.  param = suspend_lanes (k_tail: 8; 0 never parks).
                stats_out[0] / [1] = rays parked at least once / at least twice.
     WAVE       trace_closest4_wave, one ray per wave; a ray it abandons (prim = -2: wave stack overrun) is walked again by one lane with
                trace_closest4<false, true, false>, as in k_tail.  param = 1: a wave stack of one row (64 entries) instead of the render's
                24.  stats_out[0] = rays that took the fallback, [1] = steps of the wave-wide walks.
     KTRACE     the rays become the paths of a PathState and go through the real k_trace of the scene's kernel family, launched as
                renderBatch launches a first bounce (all paths queued, no sort), SMALL exactly when a render of this context would use
                it; the records are filled from its P.hit.  param = workgroups (0: one per 1024 rays, so that lanes replace their rays).
                k_trace rescales a mint that equals PPG_EPSILON (1e-4f) exactly by max(|o|_inf, 1e-4), as Scene::rayIntersect does:
                pass the scaled value to compare with the other modes.
   In every mode stats_out[2] = the entries of the scene's top cut (DevScene::n_top; 0: the wave traversal starts at the root) and
   stats_out[3] = 1 where KTRACE ran the SMALL kernel.  LANE_ANY fills prim (>= 0: occluded) and t only.  The record has no room for the
   barycentrics: p, the frame and wi are functions of (prim, u, v) and the ray, so records that are equal byte for byte stand for them. */
enum {
    PPG_DEBUG_TRACE_LANE = 0, PPG_DEBUG_TRACE_LANE_ANY = 1, PPG_DEBUG_TRACE_LANE_VOTE = 2, PPG_DEBUG_TRACE_RESUME = 3, PPG_DEBUG_TRACE_WAVE = 4,
    PPG_DEBUG_TRACE_KTRACE = 5
};
int ppg_debug_intersect_mode(struct ppg_ctx *ctx, uint32_t n, const float *rays, struct ppg_debug_hit *out, int32_t mode, int32_t param, uint32_t *stats_out);

/* emitter_sample_direct of the FULL kernels, sample by sample: per item a reference point ref[3], its normal ref_n[3] and the 2-D sample
   u[2].  Out: the emitter chosen (the hook repeats the render's pmf_sample on the same table and sample: the record does not carry the
   index), and of its direct-sampling record the direction d, the distance, the emitter's normal n, the density in
   solid angle (0 where the facing tests fail), the emitter-choice probability and value = radiance / pdf.  ppg_debug_direct_ex, the record
   of ppg_debug_sample_direct_as, adds what the render reads of the record besides: the direction sd and length sdist of the shadow ray (Scene::evalTransmittance recomputes them from the two end
   points, scene.cpp:621-623) and whether the emitter is the environment emitter (is_env) or a point / spot / directional one (is_delta).
   The record is what the device function left in its DirectSample, also for a failed sample (pdf = 0), of which the render reads nothing:
   an emitter without triangles, a missed bounding sphere and a failed envmap sample leave all of it 0 but em_pdf (and is_env); a failed
   facing test leaves the sampled point's d, dist, n, sd, sdist.  ppg_debug_sample_direct runs emitter_sample_direct<true> of the shapes
   family, whatever the scene.

   ppg_debug_sample_direct_as runs emitter_sample_direct<full != 0> as the TRACE unit of kernel family `family` (0 .. 5, csrc/ppg_device.h)
   compiled it: every family holds its own copy of the function, and a render calls the one of its scene's family.  full = 0 exists in
   the base family only (a scene of diffuse, two-sided diffuse and mirror materials; it knows no delta emitters, no environment map and no
   shapes: the host gives it no scene that holds one).  family = -1: the family and the FULL setting a render of this context's scene
   would use (`full` is ignored).  PPG_ERR_INVALID for an instantiation that does not exist — full = 0 above the base family — and for one
   that cannot read the scene: a family below the scene's own, or full = 0 for a scene whose render is FULL.
   ref and ref_n may be any floats; u is a sample, 0 <= u <= 1 (ppg_rand returns at most 1 - 2^-23), and both hooks check that on the host
   (PPG_ERR_INVALID names the first item outside, NaN included): every table index the functions form is clamped or wrapped for such a
   value (pmf_sample, envmap_sample_reuse, envmap_texel, envmap_clamp_row), while a u.y above 1 would step pmf_sample's forward skip past a
   last triangle of area 0 and read one entry beyond the emitter's tables.
   The oracle has the same entry without the two selectors, ppgo_debug_sample_direct (oracle/ppg_oracle.h): Scene::sampleEmitterDirect up to
   the shadow ray.  It fills the same record, which the device must equal bit for bit. */
struct ppg_debug_direct {
    int32_t emitter;
    float d[3];
    float dist;
    float n[3];
    float pdf, em_pdf;
    float value[3];
    float _pad[3];
};  /* 64 bytes */
struct ppg_debug_direct_ex {  /* ppg_debug_direct (its first 52 bytes), then the rest of the DirectSample */
    int32_t emitter;
    float d[3];
    float dist;
    float n[3];
    float pdf, em_pdf;
    float value[3];
    float sd[3];
    float sdist;
    int32_t is_env, is_delta;
    int32_t _pad;
};  /* 80 bytes */
int ppg_debug_sample_direct(struct ppg_ctx *ctx, uint32_t n, const float *ref, const float *ref_n, const float *u, struct ppg_debug_direct *out);
int ppg_debug_sample_direct_as(struct ppg_ctx *ctx, int32_t family, int32_t full, uint32_t n, const float *ref, const float *ref_n, const float *u,
                               struct ppg_debug_direct_ex *out);

/* The other half of multiple importance sampling: the density next-event estimation would have had for an emitter that a BSDF-sampled
   ray found — the FL_PENDING branch of k_shade / k_tail (csrc/ppg_kernels.h shade_one; GP:2078-2111), ray by ray.  rays as for
   ppg_debug_intersect (mint as it stands: Scene::rayIntersect scales a mint of exactly 1e-4f by max(|o|_inf, 1e-4), pass the scaled
   value); ref_n[3 i ..] = the normal of the DirectSamplingRecord of the vertex the ray left, three zeros = it has none (a BSDF with a
   back side or transmission).  One lane per ray runs the closest hit and the intersection record of ppg_debug_intersect (fill_isect_full:
   the mesh's shading normal; the render's fill_isect_tex gives the same normal, since bump and normal maps perturb the frame the BSDF is
   queried in, not Intersection::shFrame.n, which AreaLight::eval and pdfDirect read), eval_Le of the hit,
   or — the ray left the scene — env_fill_direct and env_radiance; then, from ref_n exactly as the render keeps them across the bounce,
   FL_PEND_REFN = dot(d, ref_n) >= 0 and nee_cos = dot(d, ref_n) (-2 without a ref_n), and with them emitter_pdf_direct, the function the
   render calls (csrc/ppg_device.h).  Like the render it asks for the density only where value is not zero: pdf_direct = 0 elsewhere.
   The search for an emitter behind null surfaces (GP:2184-2245) is not followed: the hook stops at the first hit.
     family  0 .. 5: the TRACE unit of that kernel family, FULL; -1: the scene's own.  PPG_ERR_INVALID below the scene's own.
     prim    as ppg_debug_intersect (-1: the ray left the scene; the oracle's is the triangle's index in the scene, not in leaf order)
     emitter the emitter found, as an index of the selection table (area emitters, delta emitters, the environment emitter last);
             -1 for none
     value   its radiance towards the ray's origin (0 from behind)
     pdf_direct   Emitter::pdfDirect, solid angle;  emitter_pdf = pdf_direct * the normalisation of the selection table
                  (Scene::pdfEmitterDirect, scene.cpp:949-952)
   The oracle's entry is ppgo_debug_pdf_direct: rayIntersect, Scene::Le or envFillDirectSamplingRecord + envEval, pdfEmitterDirect. */
struct ppg_debug_pdf {
    int32_t prim, emitter;
    float value[3];
    float pdf_direct, emitter_pdf;
    int32_t _pad;
};  /* 32 bytes */
int ppg_debug_pdf_direct(struct ppg_ctx *ctx, int32_t family, uint32_t n, const float *rays, const float *ref_n, struct ppg_debug_pdf *out);

/* The BSDF layer of the context's materials (after ppg_set_scene, outside a render), item by item: one small kernel of the extended
   units (csrc: PPG_MFD) whose lanes prepare the material as the render does at a hit with texture coordinates uv — the record, the bitmaps
   of ppg_material.texture / ppg_set_material_textures, the entry of ppg_set_microfacet, the coat of ppg_set_coatings (a scene with one runs the hook's kernel of
   the coat units, PPG_COAT), the blend of ppg_set_blends with its children prepared likewise at uv (the kernel of the blend units, PPG_BLEND) — and call the render's own mat_eval / mat_pdf / mat_sample on it.  A material without a general entry runs through the same functions with alphaV = alphaU, its own ggx / beckmann and
   visible sampling: the float operations of the isotropic path, which the tests hold to the oracle bit for bit.
   Per item: the material, local wi, local wo (eval / pdf), the 2-D sample, and the extra number roughdielectric::sample draws from the
   path's sampler (roughdielectric.cpp:553), named as the render names it: it is ppg_rand(key, 0) (include/ppg_rng.h).
   Out: eval = f * |cos theta_o| as the render uses it, pdf, then of mat_sample the direction, its pdf, the weight, eta and the delta /
   null flags. */
struct ppg_debug_bsdf_item {
    int32_t material;
    float wi[3], wo[3];
    float sample[2];
    uint32_t key;
    float uv[2];
};  /* 48 bytes */
struct ppg_debug_bsdf_out {
    float eval[3];
    float pdf;
    float wo[3];
    float sampled_pdf;
    float weight[3];
    float eta;
    int32_t delta, is_null;
    int32_t _pad[2];
};  /* 64 bytes */
int ppg_debug_bsdf(struct ppg_ctx *ctx, uint32_t n, const struct ppg_debug_bsdf_item *items, struct ppg_debug_bsdf_out *out);

/* The same items and record through ONE compiled copy of the BSDF layer.  mat_eval / mat_pdf / mat_sample are compiled into every kernel
   family (csrc/ppg_device.h: the families differ by preprocessor — PPG_MFD, PPG_COAT with the nested BSDF behind real calls, PPG_BLEND with
   the scene as a further argument), the base family also holds the lean bsdf_eval / bsdf_pdf / bsdf_sample and a unit compiled with
   PPG_PARAM_TEXTURES = 0, where Mat has another layout and mat_spec_lum is computed; a render calls the copies of its scene's family.
     family  0 .. 5: that kernel family; -1: the family, and FULL or LEAN, that a render of this context's scene would use (`unit` is
             ignored).
     unit    FULL    mat_eval / mat_pdf / mat_sample as the TRACE unit of `family` compiled them, the material prepared as for ppg_debug_bsdf
             LEAN    base family only: the material as the !FULL branch of shade_one loads it (the type, flags = 0, the reflectance), then
                     bsdf_eval / bsdf_pdf / bsdf_sample; eta = 1 and is_null = 0, as shade_one leaves them
             COMMON  base family only: a kernel inside the translation unit of k_shade<false, true, MSET_COMMON>, calling that unit's
                     mat_*; it looks up no bitmap on specular / alpha / opacity, as the unit never does
   _pad[0] of the record carries what the render derives from the material beside the BSDF values: bit 0 mat_is_smooth (LEAN:
   bsdf_is_smooth; only such a vertex is guided), bit 1 mat_backside_or_transmission (LEAN: the type is two-sided diffuse; such a vertex
   hands emitter sampling no normal), bit 2 mat_has_null (null surfaces are searched behind it); _pad[1] stays 0.  ppg_debug_bsdf is
   ppg_debug_bsdf_as(max(the scene's family, 2), FULL) and fills the same bits.
   PPG_ERR_INVALID, ppg_last_error naming the reason, for an instantiation that does not exist (LEAN or COMMON above the base family, an
   unknown unit or family); for one that cannot read the scene (a family below the scene's own, LEAN for a scene whose render is FULL); for
   COMMON with an item whose material sort_slice would keep out of the common part of a slice (csrc/ppg_kernels.h: a type outside diffuse /
   two-sided diffuse / mirror / conductor / roughconductor / plastic / roughplastic, a mask, a bitmap on specular / alpha / opacity, a bump
   or normal map); for a material index out of range; and — both entries — for a sample outside [0, 1], NaN included (the plug-ins divide a
   sample by a probability and index the rough-transmittance slice and a blend's cdf with the result).  PPG_ERR_STATE inside a render.  A
   refused call launches nothing.
   The oracle's entries are ppgo_bsdf_eval, ppgo_bsdf_sample_ex and ppgo_bsdf_flags (oracle/ppg_oracle.h), which every copy must equal bit
   for bit. */
enum { PPG_DEBUG_BSDF_FULL = 0, PPG_DEBUG_BSDF_LEAN = 1, PPG_DEBUG_BSDF_COMMON = 2 };
int ppg_debug_bsdf_as(struct ppg_ctx *ctx, int32_t family, int32_t unit, uint32_t n, const struct ppg_debug_bsdf_item *items,
                      struct ppg_debug_bsdf_out *out);

/* The shared float math (include/ppg_detmath.h, ppg_rng.h) as ONE module of this library compiled it; no scene is needed.  The ops, their
   arguments (bit patterns), their domains and the block checksum are those of include/ppg_mathcheck.h.
     family  0 .. 5: the TRACE unit of that kernel family (csrc/ppg_device.h) — every family's module holds its own copy of the header's
             functions and its own out-of-line dm_sincos / dm_atan2 / dm_exp / dm_log.  -1: this library's HOST code, i.e. clang's host
             pass, which compiles the tables csrc/ppg_scene_build.h bakes with ppg_exp and ppg_sincos.
     via     0: the header's functions, inlined.  1: what the kernels call — dm_sincos, dm_atan2, dm_exp, dm_log, dm_acos, dm_tan, dm_pow;
             refused (PPG_ERR_INVALID) for an op without such a copy and for family -1.
   ppg_debug_math_eval: element i of out0 / out1 receives op(a[i], b[i]); an element outside the op's domain, and out1 of an op with one
   output, keeps what the caller put there.  ppg_debug_math_checksum: out[k] = the checksum of block first_block + k of the 256 blocks of
   2^24 float patterns, for an op of one argument. */
int ppg_debug_math_eval(struct ppg_ctx *ctx, int32_t family, int32_t via, int32_t op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out0,
                        uint32_t *out1);
int ppg_debug_math_checksum(struct ppg_ctx *ctx, int32_t family, int32_t via, int32_t op, uint32_t first_block, uint32_t n_blocks, uint64_t *out);

/* EXPLICIT VERTICES through the commit of a batch: Vertex::commit (GP:1730-1768) of every vertex of every path, then the end of the round.
   Valid between ppg_begin_iteration(ctx, 0) and ppg_build_sdtree, outside ppg_render_passes; the vertices go into the context's current
   building tree and leaf headers under its spatialFilter, directionalFilter, loss, nee and do_nee (ppg_set_do_nee), through the render's
   own launchers: the hook builds a PathState from the arrays below — one small kernel finds every vertex's leaf and voxel size with
   stree_lookup, as k_shade does — and runs launchCommitKernels, reserveRoundRecords, applyAdamRound and the fold of the weight replicas.
   The optimiser's path id of path i is i (n_pix = n_paths, identity pixel list).  The oracle has the same entry, ppgo_debug_commit: there
   every vertex becomes a Vertex whose dTree is STree::dTreeWrapper(p, voxel), committed by Vertex::commit with the sampler at
   (key, dim + 3 v), and the round ends with the oracle's applyAdamRound.
     route  COMMIT          k_commit over all paths.
            COMMIT_SPLIT    k_commit with the late paths left out (their nv8 byte is 0), then k_commit over the list of the late paths: a
                            batch with a tail.
            RECORDS         k_commit_records, the sort, k_splat_sorted, k_adam_apply: a round with known record positions.  Refused unless
                            a round runs (a loss is set and the tree is built), recordPositionsKnown holds for the context and the flag
                            bit fits the key.  The route is the caller's choice: PPG_NO_SORTED_COMMIT, which makes the RENDER commit its
                            rounds with k_commit, does not change what a route of this hook runs.
            RECORDS_SPLIT   the same with the late paths through the list launch; they reserve max_vertices positions each, as a path
                            handed to k_tail does (the unused ones stay holes).
     per path    nv (0 .. max_vertices of the context), key, dim (the sampler's dimension when Li returned), late (NULL: none)
     per vertex  (n_vertices = sum nv, path after path) p, d, radiance, throughput, bsdf_val [3]; wo_pdf, bsdf_pdf, dtree_pdf; is_delta
   Out: committed (vertices Vertex::commit accepted); the valid sorted keys of a record route, "splat only" flag bit (just above the leaf
   bits) included — *n_keys is their number also when it exceeds keys_cap —; the optimiser's records in key order (likewise); and the
   optimiser's state of every S-tree node after the round, 6 words as ppg_adam_state gives them (adam_state: NULL or n_stree_nodes * 6).
   Every count and index is checked on the host (PPG_ERR_INVALID, ppg_last_error names the argument; PPG_ERR_STATE outside an iteration)
   and a refused call leaves the context as it was; PPG_ERR_STATE also while a round hook (ppg_set_pass_hook) is installed.  The floats may be anything: no kernel indexes with them. */
enum { PPG_DEBUG_COMMIT = 0, PPG_DEBUG_COMMIT_SPLIT = 1, PPG_DEBUG_COMMIT_RECORDS = 2, PPG_DEBUG_COMMIT_RECORDS_SPLIT = 3 };
struct ppg_adam_record;
struct ppg_debug_commit_in {
    int32_t route;
    uint32_t n_paths;
    uint64_t n_vertices;
    const uint32_t *nv, *key, *dim;
    const uint8_t *late;
    const float *p, *d, *radiance, *throughput, *bsdf_val;
    const float *wo_pdf, *bsdf_pdf, *dtree_pdf;
    const uint8_t *is_delta;
};
struct ppg_debug_commit_out {
    uint64_t committed;
    uint64_t n_keys, keys_cap;
    uint64_t *keys;
    uint64_t n_records, records_cap;
    struct ppg_adam_record *records;
    uint32_t *adam_state;
};
int ppg_debug_commit(struct ppg_ctx *ctx, const struct ppg_debug_commit_in *in, struct ppg_debug_commit_out *out);
/* Host only: the depth of an S-tree given as ppg_sdtree_read_stree gives it (children[2 i], children[2 i + 1]; 0, 0 = a leaf; a child's
   index is above its parent's) — levels below the root of its deepest leaf — and what the refine step answers to it under the spatial
   filter (0 nearest, 1 stochastic, 2 box): PPG_OK, or PPG_ERR_NOMEM for a tree deeper than PPG_STREE_MAX_DEPTH under the box filter.
   The box filter's splat (stree_record_box, csrc/ppg_kernels.h) walks the S-tree depth first with a stack of 96 entries: an interior
   node d levels below the root is popped with d entries left — one sibling per level above it — and pushes its two children, d + 2 <= 96.
   The 96 entries therefore serve interior nodes down to level 94, i.e. trees whose deepest leaf lies 95 levels below the root; the limit
   is set one level below that.  PPG_ERR_INVALID: a child index that is not above its parent's or beyond n_nodes. */
#define PPG_STREE_MAX_DEPTH 94
int ppg_debug_stree_depth(const uint32_t *children, uint32_t n_nodes, int32_t spatial_filter, uint32_t *depth);

/* The media family's device functions (csrc/ppg_device.h: medium_sample_distance, medium_transmittance, phase_sample, phase_eval), item by
   item, over the media of the scene that is set — which must bind a medium (include/ppg.h ppg_set_media), else PPG_ERR_STATE.  Per item:
   HomogeneousMedium::sampleDistance on a ray that starts at the origin, runs along -wi and ends after `length` (may be infinite), with
   u[0] as its first random number and u[1] as the second one where it draws one; evalTransmittance over `length`; the phase function's
   sample with (u[2], u[3]) for wi, its value and its density for the sampled direction.  t is the sampled distance as sampleDistance leaves
   it: the distance of the medium event, or `length` on failure.  PPG_ERR_INVALID: a medium index out of range, a u outside [0, 1]. */
struct ppg_debug_medium_item {
    int32_t medium;
    float length;
    float wi[3];
    float u[4];
};                                /* 36 bytes */
struct ppg_debug_medium_out {
    int32_t success;
    float t, pdf_success, pdf_failure;
    float transmittance[3];       /* mRec.transmittance */
    float eval_transmittance[3];
    float wo[3];
    float phase_eval, phase_pdf;
};                                /* 60 bytes */
int ppg_debug_medium(struct ppg_ctx *ctx, uint32_t n, const struct ppg_debug_medium_item *items, struct ppg_debug_medium_out *out);

/* The hetmedia family's device functions (csrc/ppg_device.h: volume_lookup_float / volume_lookup_rgb, hetmedium_sample_distance,
   hetmedium_transmittance), item by item, over the volumes and media of the scene that is set — which must bind a heterogeneous medium
   (include/ppg.h ppg_set_media_volumes), else PPG_ERR_STATE.
   ppg_debug_volume: the lookup of volume `volume` at the world-space point p; a one-channel volume answers in value[0] (value[1], value[2] = 0).
   ppg_debug_hetmedium: HeterogeneousMedium::sampleDistance on the ray (o, d) with mint = 0 and the given maxt (may be infinite), then
   evalTransmittance on the same ray; the random numbers are ppg_rand(key, dim), ppg_rand(key, dim + 1), ..: sampleDistance takes `draws`
   of them, evalTransmittance the next `eval_draws`.  t, sigma_s and transmittance are mRec's (t = 0 and zeros on failure); medium must name
   a heterogeneous medium.  PPG_ERR_INVALID: an index out of range, a medium that is not heterogeneous. */
struct ppg_debug_volume_item {
    int32_t volume;
    float p[3];
};                                /* 16 bytes */
struct ppg_debug_volume_out {
    float value[3];
};                                /* 12 bytes */
int ppg_debug_volume(struct ppg_ctx *ctx, uint32_t n, const struct ppg_debug_volume_item *items, struct ppg_debug_volume_out *out);
struct ppg_debug_hetmedium_item {
    int32_t medium;
    float o[3], d[3];
    float maxt;
    uint32_t key, dim;
};                                /* 40 bytes */
struct ppg_debug_hetmedium_out {
    int32_t success;
    float t;
    float sigma_s[3];
    float transmittance;
    uint32_t draws;
    float eval_transmittance;
    uint32_t eval_draws;
};                                /* 36 bytes */
int ppg_debug_hetmedium(struct ppg_ctx *ctx, uint32_t n, const struct ppg_debug_hetmedium_item *items, struct ppg_debug_hetmedium_out *out);

#ifdef __cplusplus
}
#endif
#endif /* PPG_TESTHOOKS_H */
