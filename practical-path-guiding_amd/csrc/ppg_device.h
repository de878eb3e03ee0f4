/*
 * ppg_device.h — device-side data layout and per-path building blocks of the guided path tracer.
 *
 * Layout (everything lives in HBM, flat arrays, no pointers inside nodes):
 *   triangles   3 x float4 per triangle in BVH-leaf order: (p0, material), (p1, emitter), (p2, original index)
 *   BVH2        64-byte nodes: both child boxes + child refs (one node visit = one 64 B read)
 *   S-tree      int4 per node {axis, child0, child1, 0}; child0 == 0 ⇔ leaf   (STreeNode, GP:740-845)
 *   leaf hdr    LeafHdr per S-tree node (D-tree descriptors + Adam state)      (DTreeWrapper, GP:570-738)
 *   sampling D-trees  SNode pool: float sum[4] + u16 child[4] + pad = 32 B     (QuadTreeNode, GP:158-371)
 *   building D-trees  bchild pool (u16x4) + bacc pool (u64x4 fixed point), index-aligned with the SNode
 *                     pool of the next iteration
 * GP:n = /root/reference/mitsuba/src/integrators/path/guided_path.cpp:n.
 *
 * All floating-point expressions are written out operation by operation (no FMA contraction, no libm)
 * so that the result of every path is bit-identical to the CPU oracle given the same sampler key.
 */
#ifndef PPG_DEVICE_H
#define PPG_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ppg_detmath.h"
#include "../../include/ppg_rng.h"
#include "../../include/ppg.h"

#define D __device__ __forceinline__
// The large path kernels — k_trace, k_shade, k_tail — are compiled once per kernel FAMILY: a translation unit is built with -DPPG_FAMILY=f
// (ppg_inst.hip), a family holds every feature of the families below it, and a scene runs the lowest family that has all it needs
// (sceneFamily, ppg_hip.hip).  Each feature costs registers the FULL kernels do not have — one more analytic test behind each traversal,
// say —, so no scene pays for one it does not use.  Everything a family adds sits under its feature macro, and its kernels' symbols are
// the names with its suffix: k_trace_shapes, k_shade_ext, k_tail_coat.
#define PPG_FAMILY_BASE 0    //           every scene without what follows
#define PPG_FAMILY_SHAPES 1  // _shapes   analytic disks and cylinders (ppg_set_shapes)
#define PPG_FAMILY_EXT 2     // _ext      the general MicrofacetDistribution (ppg_set_microfacet: alphaU / alphaV, Phong / Ashikhmin-Shirley,
                             //           sampleVisible = false), with or without analytic shapes
#define PPG_FAMILY_COAT 3    // _coat     the coating / roughcoating adapters (ppg_set_coatings), whatever else the scene holds
#define PPG_FAMILY_BLEND 4   // _blend    the blendbsdf / mixturebsdf combinators (ppg_set_blends), whatever else the scene holds
#define PPG_FAMILY_LOBES 5   // _lobes    the roughdiffuse, difftrans and phong BSDFs (PPG_BSDF_ROUGHDIFFUSE ..), whatever else the scene holds; being the top
                             //           family it also compiles the normalmap adapter and the null BSDF (PPG_NORMALMAP_NULL)
#define PPG_FAMILY_MEDIA 6   // _media    homogeneous participating media (ppg_set_media with a binding), whatever else the scene holds
#define PPG_FAMILY_HETMEDIA 7  // _hetmedia  heterogeneous participating media (ppg_set_media_volumes names a bound medium), whatever else the scene holds: now the top family
#define PPG_FAMILIES 8
#define PPG_DEBUG_FAMILIES 6  // the families whose copies the item-by-item test hooks address by number (the media family adds nothing to that code)
#define PPG_SUFFIX_0
#define PPG_SUFFIX_1 _shapes
#define PPG_SUFFIX_2 _ext
#define PPG_SUFFIX_3 _coat
#define PPG_SUFFIX_4 _blend
#define PPG_SUFFIX_5 _lobes
#define PPG_SUFFIX_6 _media
#define PPG_SUFFIX_7 _hetmedia
#ifndef PPG_FAMILY
#define PPG_FAMILY 0  // (a digit: it is pasted to PPG_SUFFIX_)
#endif
#define PPG_SHAPES (PPG_FAMILY >= PPG_FAMILY_SHAPES)
#define PPG_MFD (PPG_FAMILY >= PPG_FAMILY_EXT)
#define PPG_COAT (PPG_FAMILY >= PPG_FAMILY_COAT)
#define PPG_BLEND (PPG_FAMILY >= PPG_FAMILY_BLEND)
#define PPG_LOBES (PPG_FAMILY >= PPG_FAMILY_LOBES)
#define PPG_MEDIA (PPG_FAMILY >= PPG_FAMILY_MEDIA)
#define PPG_HETMEDIA (PPG_FAMILY >= PPG_FAMILY_HETMEDIA)
// the normalmap adapter (PPG_MAT_NORMALMAP) and the null BSDF (PPG_BSDF_NULL): no family of their own — the top family, which holds
// everything below it, compiles them, and sceneFamily sends a scene with either there
#define PPG_NORMALMAP_NULL (PPG_FAMILY >= PPG_FAMILY_LOBES)
#define PPG_CAT2(a, b) a##b
#define PPG_CAT(a, b) PPG_CAT2(a, b)
#define PPG_FAMILY_NAME(name) PPG_CAT(name, PPG_CAT(PPG_SUFFIX_, PPG_FAMILY))
#define k_trace PPG_FAMILY_NAME(k_trace)
#define k_shade PPG_FAMILY_NAME(k_shade)
#define k_tail PPG_FAMILY_NAME(k_tail)

struct F3 {
    float x, y, z;
};
D F3 f3(float x, float y, float z) { F3 r; r.x = x; r.y = y; r.z = z; return r; }
D F3 f3s(float v) { return f3(v, v, v); }
D F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
D F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
D F3 operator*(F3 a, float f) { return f3(a.x * f, a.y * f, a.z * f); }
D F3 operator-(F3 a) { return f3(-a.x, -a.y, -a.z); }
D F3 mul3(F3 a, F3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }
D F3 div3(F3 a, float f) { float r = 1.0f / f; return f3(a.x * r, a.y * r, a.z * r); }  // vector.h:535-542
D float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D F3 cross3(F3 a, F3 b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
D float len3(F3 v) { return __builtin_sqrtf(dot3(v, v)); }
D F3 norm3(F3 v) { return div3(v, len3(v)); }  // vector.h:625-627
D float comp3(F3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
D bool iszero3(F3 s) { return s.x == 0.0f && s.y == 0.0f && s.z == 0.0f; }
D bool isvalid3(F3 s) {  // spectrum.h:467-472
    return ppg_isfinite(s.x) && !(s.x < 0.0f) && ppg_isfinite(s.y) && !(s.y < 0.0f) && ppg_isfinite(s.z) && !(s.z < 0.0f);
}
D float avg3(F3 s) { float r = 0.0f; r += s.x; r += s.y; r += s.z; return r * (1.0f / 3); }  // spectrum.h:481-486
D float max3(F3 s) { return ppg_max(ppg_max(s.x, s.y), s.z); }
D F3 ld3(const float4 *p) { float4 v = *p; return f3(v.x, v.y, v.z); }

// ------------------------------------------------------------------------------------------------
// include/ppg_detmath.h on the device: ONE out-of-line copy of each transcendental per kernel module instead of one inlined copy per
// call site.  Pure register-in / register-out functions (no pointers: nothing is forced into scratch memory); the arithmetic is the
// header's, so results are unchanged.  Inlined everywhere they were 4 400 of k_tail<FULL>'s 25 000 instructions — a kernel of 135 KB
// (330 KB before the BSDF call sites were merged) against a 64 KB instruction cache.
// ------------------------------------------------------------------------------------------------
#define DM_ATTR static __device__ __attribute__((noinline))
DM_ATTR float2 dm_sincos(float x) { float s_, c_; ppg_sincos(x, &s_, &c_); return make_float2(s_, c_); }
DM_ATTR float dm_atan2(float y, float x) { return ppg_atan2(y, x); }
DM_ATTR float dm_exp(float x) { return ppg_exp(x); }
DM_ATTR float dm_log(float x) { return ppg_log(x); }
D void dm_sincos(float x, float *s, float *c) { const float2 r = dm_sincos(x); *s = r.x; *c = r.y; }
D float dm_acos(float x) { return dm_atan2(__builtin_sqrtf(ppg_max(0.0f, (1.0f - x) * (1.0f + x))), x); }  // = ppg_acos
D float dm_tan(float x) { const float2 r = dm_sincos(x); return r.x / r.y; }                                 // = ppg_tan
D float dm_pow(float x, float y) { return dm_exp(y * dm_log(x)); }                                            // = ppg_pow

// ------------------------------------------------------------------------------------------------
// Scene
// ------------------------------------------------------------------------------------------------
struct BvhNode {  // 64 B
    float lo0[3], hi0[3], lo1[3], hi1[3];
    int c0, c1;   // n > 0: first triangle (leaf-order index); n == 0: node index
    int n0, n1;   // > 0 leaf with n triangles, 0 interior, < 0 empty
};

// BVH4 node, 128 B = one L2 line: child boxes in SoA (six float4 loads in flight at once), then child refs.
// child >= 0: interior node index; child < 0: leaf, ~child = (first triangle << 3) | (count - 1); an unused
// slot is marked PPG_BVH4_EMPTY.
#define PPG_BVH4_EMPTY 0x7fffffff
struct Bvh4Node {  // host-side intermediate of the builder
    float lox[4], loy[4], loz[4], hix[4], hiy[4], hiz[4];
    int child[4];
    int pad[4];
};
// What the kernels traverse: the same node in 64 B (four 16-byte loads instead of seven).  The child boxes are quantised to 8 bits per
// coordinate on a grid spanned by the node's own lower corner and a power-of-two cell size per axis: lo = origin + qlo * 2^e (rounded
// down at build time), hi = origin + qhi * 2^e (rounded up) — every decoded box CONTAINS the builder's padded float box (checked by
// the builder in the device's float arithmetic), so culling stays conservative and the closest hit is unchanged.
struct __attribute__((aligned(16))) Bvh4QNode {
    float ox, oy, oz;
    unsigned int exps;                     // byte a (0, 1, 2): biased exponent of the cell size along axis a, i.e. the float with bits (byte << 23)
    unsigned int qlox, qloy, qloz, qhix;   // child k in byte k
    unsigned int qhiy, qhiz;
    int child[4];
    int pad[2];
};
// decode one node: child boxes as floats, child refs
D void bvh4q_load(const Bvh4QNode *node, float lxs[4], float lys[4], float lzs[4], float hxs[4], float hys[4], float hzs[4], int chs[4]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(node);
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
    const float ox = __uint_as_float(a.x), oy = __uint_as_float(a.y), oz = __uint_as_float(a.z);
    const float sx = __uint_as_float((a.w & 255u) << 23), sy = __uint_as_float(((a.w >> 8) & 255u) << 23), sz = __uint_as_float(((a.w >> 16) & 255u) << 23);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lxs[k] = ox + (float)((b.x >> (8 * k)) & 255u) * sx;
        lys[k] = oy + (float)((b.y >> (8 * k)) & 255u) * sy;
        lzs[k] = oz + (float)((b.z >> (8 * k)) & 255u) * sz;
        hxs[k] = ox + (float)((b.w >> (8 * k)) & 255u) * sx;
        hys[k] = oy + (float)((c.x >> (8 * k)) & 255u) * sy;
        hzs[k] = oz + (float)((c.y >> (8 * k)) & 255u) * sz;
    }
    chs[0] = (int)c.z; chs[1] = (int)c.w; chs[2] = (int)d.x; chs[3] = (int)d.y;
}

struct DevCamera {
    float s2c[16], c2w[16];
    float near_clip, far_clip, inv_w, inv_h;
    int width, height;
    int lens;                 // thin lens (ppg_set_lens): 0 = pinhole
    float aperture, focus;    // its aperture radius and focus distance
};

#define PPG_MAT_STRIDE 6  // float4 per material: (reflectance, type) (specular, alpha) (eta, flags) (k, fdrInt) (opacity, rtrans slice) (texture word, specular / alpha / opacity texture: 1 + index as bits, 0 = none)

// ppg_texture on the device: texels as (rgb, -)
struct DevTex {
    const float4 *texels;
    int w, h;
    float su, sv, ou, ov;
    int wrap_u, wrap_v, nearest, pad;
};

struct DevScene {
    const float4 *tris;     // 3 per triangle: positions (.w = material, emitter, original index) — intersection records only
    const float4 *accel;    // 3 per triangle: TriAccel (triaccel.h:36-58), what the traversal reads
    const float4 *accel_small;  // small scenes (brute force from LDS): the same records sorted by projection axis k,
    int small_n[3];             // n[k] of them per axis (degenerate triangles dropped); record[2].z = leaf-order index
    const float4 *normals;  // 3 per triangle or nullptr
    const BvhNode *bvh;
    const Bvh4QNode *bvh4;    // same tree collapsed to 4-wide nodes with quantised child boxes (generic traversal)
    const float4 *bvh_top;    // its top cut for trace_closest4_wave: n_top <= 64 subtrees, (lo, child ref) (hi, -) each; n_top == 0: start at the root
    int n_top;
    const float4 *materials;  // (reflectance rgb, type)
    const float4 *emitters;   // (radiance rgb, -)
    int n_tris;
    DevCamera cam;
    // next-event estimation: one area emitter = the triangles carrying its id, in index order
    int has_null;              // some BSDF has a null (pass-through) component: the look-through code of the FULL kernels is live
    float4 env;                // constant environment emitter (constant.cpp): radiance rgb, w != 0 if present (FULL kernels only);
    float4 bsphere;            // its bounding sphere (constant.cpp:67-78): centre, radius; it is emitter number n_emitters
    int n_emitters;            // area emitters
    const float *em_sel_cdf;   // [n_emitters (+ 1 with an environment emitter) + 1] emitter pmf (Scene::configure, samplingWeight = 1)
    float em_sel_norm;         // DiscreteDistribution::getNormalization()
    const int4 *em_info;       // (first triangle, triangle count, first cdf entry, invSurfaceArea bits)
    const float *em_area_cdf;  // per emitter: count + 1 entries (TriMesh::prepareSamplingTable)
    const float4 *em_tris;     // 3 per emitter triangle: positions
    const float4 *em_normals;  // 3 per emitter triangle or nullptr
    const float *rtrans;       // roughplastic: rough-transmittance slices, rtrans_n + 1 floats each (ppg_scene.rtrans)
    int rtrans_n;
    // analytic spheres (FULL kernels, BVH path only): 4 float4 each = (centre, radius) (R row 0, material) (R row 1, emitter)
    // (R row 2, flip normals); primitive numbers n_tris, n_tris + 1, ..
    const float4 *spheres;
    int n_spheres;
    // image-based environment emitter (envmap.cpp), env.w == 2: texels (rgb, -), the row / column cdfs and sin(theta) row weights
    // of EnvironmentMap::configure, m_normalization, m_scale, the pixel size in spherical coordinates, toWorld's rotation
    const float4 *em_texels;
    const float *em_cdf_rows, *em_cdf_cols, *em_row_weights;
    int em_w, em_h;
    float em_norm, em_scale, em_px, em_py;
    float em_R[9];
    // bitmap textures (FULL kernels): texture coordinates, 3 x float2 per triangle in leaf order (NaN = the mesh has none) or nullptr
    const float2 *uvs;
    const DevTex *textures;
    // delta emitters (ppg_set_delta_emitters; FULL kernels): PPG_DELTA_STRIDE float4 each = (intensity rgb, type) (position or direction,
    // cutoff angle) (row 2 of the world-to-light rotation, 1 / (cutoff - beam width)) (cos cutoff, cos beam width, -, -); they are emitters
    // n_emitters .. n_emitters + n_delta - 1, and the environment emitter is number n_emitters + n_delta
    const float4 *delta;
    int n_delta;
    // ppg_set_blends with a blended material (blend kernels only, PPG_BLEND): PPG_BLEND_STRIDE float4 = 16 words per material — the
    // children (4 material indices), the eval weights (4), the normalised cdf (5: DiscreteDistribution::m_cdf), the PPG_BLENDF_* bits,
    // the weight texture (1 + index), 0; nullptr otherwise.  (It stands here, in the padding in front of the next float4, so that no
    // other member and no kernel argument behind the scene moves: the kernels of the other families stay what they were.)
    const float4 *blend;
    float4 dir_sphere;         // DirectionalEmitter::m_bsphere: the geometry box's bounding sphere, radius * 1.1 (directional.cpp:88-94)
    // analytic disks and cylinders (ppg_set_shapes; FULL kernels, BVH path only): PPG_SHAPE_STRIDE float4 each = rows 0..2 of the 3x4
    // object-to-world, rows 0..2 of its inverse, (radius, length, invSurfaceArea, type) (material, emitter, flip normals, -); primitive
    // numbers n_tris + n_spheres, ..
    const float4 *shapes;
    int n_shapes;
    // a material is a roughdiffuse, difftrans or phong lobe: the scene runs the lobes kernels (PPG_LOBES), which alone compile them.  (It
    // stands in the padding behind n_shapes: no other member and no kernel argument behind the scene moves.)  Bit 0: such a lobe; bit 1: a
    // normal-mapped or null material (PPG_NORMALMAP_NULL), which the same kernels alone compile.  No kernel reads it.
    int lobes;
    // ppg_set_microfacet with a general entry (extended kernels only, PPG_MFD): one float4 per material = (alphaV, PPG_MFDF_* bits,
    // alphaV texture: 1 + index as bits, -); nullptr otherwise
    const float4 *mfd;
    // ppg_set_coatings with a coat (coat kernels only, PPG_COAT): PPG_COAT_STRIDE float4 per material = (eta, thickness,
    // specularSamplingWeight, PPG_COATF_* bits), (sigmaA, alpha), (specularReflectance, rough-transmittance slice as int); nullptr otherwise
    const float4 *coat;
};
// ppg_set_media with a binding: what the media kernels (PPG_MEDIA) get on top of DevScene and PathState.  The kernels of the other families
// keep their arguments — and with them their code — as they are: the host carries this record beside the scene (ppg_launch.h), and the
// launchers of the media family append it to the two structs (SceneArg here, PathArg in ppg_kernels.h).
//   media       PPG_MEDIUM_STRIDE float4 per medium = (sigmaS, mediumSamplingWeight) (sigmaT, samplingDensity) (g, strategy, phase, -)
//   prim_media  one binding word per primitive — triangles in LEAF order, then the spheres, then the shapes —: low 16 bits = 1 + interior
//               medium, high 16 bits = 1 + exterior medium, 0 = no transition
//   camera_medium  1 + the medium the sensor lies in, 0 = none
//   path_medium, path_stride  the paths' medium words (PathArg::medium); nullptr everywhere: the scene binds no medium
struct MediaArgs {
    const float4 *media;
    const unsigned int *prim_media;
    unsigned int camera_medium;
    int n_media;
    unsigned int *path_medium;
    unsigned int path_stride;
};
// ppg_set_media_volumes with a bound heterogeneous medium: what the hetmedia kernels (PPG_HETMEDIA) get on top of MediaArgs, carried and
// appended the same way (the media family's kernels, ppg_debug_medium's among them, keep MediaArgs as it is).
//   volumes  PPG_VOLUME_STRIDE float4 per volume = (kind | channels << 8, res x, res y, res z as ints) (worldToGrid rows 0, 1, 2: an affine 3x4)
//            (value r, g, b; the grid's first float in `pool` as an int)
//   pool     the grids' float32 data, one after the other, each in the reference's order ((z * ry + y) * rx + x) * channels + c
//   het      PPG_HET_STRIDE float4 per medium = (1 + density volume, 0 = a homogeneous medium; albedo volume; scale; invMaxDensity)
//            (the density's world box min, -) (its max, -): the reference's default box (+inf, -inf) for a const density
struct HetArgs {
    const float4 *volumes;
    const float *pool;
    const float4 *het;
    int n_volumes;
};
#if PPG_HETMEDIA
struct DevSceneMedia : DevScene {
    const float4 *media;
    const unsigned int *prim_media;
};
struct DevSceneHet : DevSceneMedia {
    const float4 *volumes;
    const float *pool;
    const float4 *het;
};
typedef DevSceneHet SceneArg;
#elif PPG_MEDIA
struct DevSceneMedia : DevScene {
    const float4 *media;
    const unsigned int *prim_media;
};
typedef DevSceneMedia SceneArg;
#else
typedef DevScene SceneArg;
#endif
#define PPG_MEDIUM_STRIDE 3
#define PPG_VOLUME_STRIDE 5
#define PPG_HET_STRIDE 3
#define PPG_HETMEDIUM_STEP_CAP 65536  // a tracking loop's steps: sixteen times the host's bound on their mean (PPG_HETMEDIUM_MAX_MEAN_STEPS); reaching it ends the segment as opaque
#define PPG_BLEND_STRIDE 4
#define PPG_BLENDW_CHILD 0        // word offsets into a material's 16 words
#define PPG_BLENDW_WEIGHT 4
#define PPG_BLENDW_CDF 8
#define PPG_BLENDW_BITS 13
#define PPG_BLENDW_TEX 14
#define PPG_BLENDF_KIND 3u        // 0 none, 1 blendbsdf, 2 mixturebsdf
#define PPG_BLENDF_N_SHIFT 2      // bits 2..4: the number of children
#define PPG_BLENDF_TEXTURED 32u   // the weight or a child reads a bitmap, or a child is anisotropic: the hit needs its.uv and the UV tangents
#define PPG_BLENDF_SMOOTH 64u     // a child has a smooth component (getType() & ESmooth)
#define PPG_COAT_STRIDE 3
#define PPG_COATF_KIND 3u         // 0 none, 1 coating, 2 roughcoating
#define PPG_COATF_TYPE_SHIFT 2    // bits 2..3: MFD_BECKMANN / MFD_GGX / MFD_PHONG of a roughcoating
#define PPG_COATF_SAMPLE_ALL 16u  // roughcoating: sampleVisible = false (always with phong)
#define PPG_MFDF_GENERAL 1u     // the entry is live
#define PPG_MFDF_PHONG 2u       // distribution = phong / as
#define PPG_MFDF_SAMPLE_ALL 4u  // sampleVisible = false (always with PHONG)
#define PPG_MFDF_ANISO 8u       // alphaU != alphaV or either comes from a bitmap: the shading frame follows the UV tangents (trimesh.cpp:380)
#define PPG_DELTA_STRIDE 4
#define PPG_SHAPE_STRIDE 8

struct Hit {
    float t, u, v;
    int prim;  // leaf-order triangle index, -1 = miss
};

// TriAccel::rayIntersect (triaccel.h:99-195) — Wald's pre-projected triangle test, the one Mitsuba's kd-tree leaves run;
// identical arithmetic to the oracle's.  A = 3 float4: (n_u, n_v, n_d, k) (a_u, a_v, b_nu, b_nv) (c_nu, c_nv, -, original index).
// Every lane of a wave tests the same triangle in the brute-force loop, so the switch on k is wave-uniform there.
// The test on a record that is in registers; the arithmetic of TriAccel::rayIntersect in its order.
D bool tri_hit_regs(const float4 a0, const float4 a1, const float4 a2, F3 o, F3 d, float mint, float maxt, float &tt, float &uu, float &vv) {
    const int k = __float_as_int(a0.w);
    // (selects, not three divergent blocks of moves: the lanes of a wave test unrelated triangles; measured equal on KITCHEN, less code)
    if ((unsigned int)k > 2u) return false;
    const bool k0 = k == 0, k1 = k == 1;
    const float o_u = k0 ? o.y : (k1 ? o.z : o.x), o_v = k0 ? o.z : (k1 ? o.x : o.y), o_k = k0 ? o.x : (k1 ? o.y : o.z);
    const float d_u = k0 ? d.y : (k1 ? d.z : d.x), d_v = k0 ? d.z : (k1 ? d.x : d.y), d_k = k0 ? d.x : (k1 ? d.y : d.z);
    const float t = (a0.z - o_u * a0.x - o_v * a0.y - o_k) / (d_u * a0.x + d_v * a0.y + d_k);
    if (t < mint || t > maxt) return false;
    const float hu = o_u + t * d_u - a1.x;
    const float hv = o_v + t * d_v - a1.y;
    const float u = hv * a1.z + hu * a1.w;
    const float v = hu * a2.x + hv * a2.y;
    if (!(u >= 0 && v >= 0 && u + v <= 1.0f)) return false;
    tt = t; uu = u; vv = v;
    return true;
}
// The three words of a record are fetched TOGETHER and waited for once: left to itself the compiler sinks each load to its first use
// behind the test's early-outs, which made a triangle four dependent memory round trips — projection axis, plane equation, edges,
// original index (ISA of round 3's k_trace; even as L1 hits that is four waits of a wave's slowest lane per leaf).  orig = a2.w.
#define PPG_PIN4(v) asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w))
D bool tri_hit(const float4 *A, F3 o, F3 d, float mint, float maxt, float &tt, float &uu, float &vv, int &orig) {
    float4 a0 = A[0], a1 = A[1], a2 = A[2];
    PPG_PIN4(a0); PPG_PIN4(a1); PPG_PIN4(a2);
    orig = __float_as_int(a2.w);
    return tri_hit_regs(a0, a1, a2, o, d, mint, maxt, tt, uu, vv);
}

// The same test with the projection axis known at compile time (small scenes: triangles are grouped by axis, so the
// component selection is hoisted out of the loop).  (o_u, o_v, o_k) / (d_u, d_v, d_k) are already permuted.
D bool tri_hit_axis(const float4 *A, float o_u, float o_v, float o_k, float d_u, float d_v, float d_k, float mint, float maxt, float &tt,
                    float &uu, float &vv) {
    const float4 a0 = A[0];
    const float t = (a0.z - o_u * a0.x - o_v * a0.y - o_k) / (d_u * a0.x + d_v * a0.y + d_k);
    if (t < mint || t > maxt) return false;
    const float4 a1 = A[1];
    const float hu = o_u + t * d_u - a1.x;
    const float hv = o_v + t * d_v - a1.y;
    const float u = hv * a1.z + hu * a1.w;
    const float4 a2 = A[2];
    const float v = hu * a2.x + hv * a2.y;
    if (!(u >= 0 && v >= 0 && u + v <= 1.0f)) return false;
    tt = t; uu = u; vv = v;
    return true;
}

D float safe_inv(float d) { return d == 0.0f ? 1e30f : 1.0f / d; }

// Scene cache in LDS: the first `n_nodes` BVH nodes and (if they all fit) the triangles.  Small scenes such
// as CBOX live there entirely; for large ones the top of the tree, which every ray visits, does.
struct LdsScene {
    const BvhNode *nodes;
    const float4 *tris;
    int n_nodes, n_tris;
};

// Traversal stack: the first PPG_LDS_STACK entries of every lane live in an LDS column (conflict-free, no
// scratch traffic), deeper entries — rare — in a small private array.
#ifndef PPG_LDS_STACK
#define PPG_LDS_STACK 24
#endif
#define PPG_STACK_OVER (48 - PPG_LDS_STACK)  // entries of a lane's overflow array: LDS column + overflow = 48 entries, whatever the split
#ifndef PPG_LEAF_VOTE_TAIL
#define PPG_LEAF_VOTE_TAIL 16  // leaf vote of k_tail's traversals (trace_closest4<.., VOTE>, trace_closest4_resume).  8 until leaves held up to 4 triangles
                               // and a wave's last traversals were suspended (round 6: 16 +0.8 %, 24 +0.4 % on the driver's command)
#endif
// (the overflow array is a separate object: as a member it kept the whole struct — stack pointer included — in scratch memory, and
// every push / pop went through a scratch load and store)
struct TStack {
    int *lds;      // this lane's column, stride blockDim.x
    int stride;
    int *over;     // int[48 - cap] of the caller
    int sp;
    int cap;       // rows of the LDS column (PPG_LDS_STACK; k_trace: PPG_TRACE_STACK) — a constant after inlining
    D void push(int v) { if (sp < cap) lds[sp * stride] = v; else over[sp - cap] = v; ++sp; }
    D int pop() { --sp; return sp < cap ? lds[sp * stride] : over[sp - cap]; }
    // the children of a node that were hit, farthest first (c1 ends on top): one range check for all three instead of one per push
    D void push_children(int m, int c1, int c2, int c3) {
        if (sp + 3 <= cap) {
            int *q = lds + sp * stride;
            if (m > 3) { *q = c3; q += stride; }
            if (m > 2) { *q = c2; q += stride; }
            if (m > 1) *q = c1;
            sp += m - 1;
            return;
        }
        if (m > 3) push(c3);
        if (m > 2) push(c2);
        if (m > 1) push(c1);
    }
};

// solveQuadraticDouble (util.cpp:487-525)
D bool solve_quadratic_double(const double A, const double B, const double C, double &nearT, double &farT) {
    if (A == 0) {
        if (B != 0) nearT = farT = -C / B;
        else return false;
    } else {
        const double discrim = B * B - 4.0f * A * C;
        if (discrim < 0) return false;
        double temp;
        const double sqrtDiscrim = __builtin_sqrt(discrim);
        if (B < 0) temp = -0.5f * (B - sqrtDiscrim);
        else temp = -0.5f * (B + sqrtDiscrim);
        nearT = temp / A;
        farT = C / temp;
        if (nearT > farT) { const double sw = nearT; nearT = farT; farT = sw; }
    }
    return true;
}
// Sphere::rayIntersect (sphere.cpp:164-189) with solveQuadraticDouble: double precision, like the reference
D bool sphere_hit(const float4 c, F3 ro, F3 rd, float mint, float maxt, float &t) {
    const double ox = (double)ro.x - (double)c.x, oy = (double)ro.y - (double)c.y, oz = (double)ro.z - (double)c.z;
    const double dx = rd.x, dy = rd.y, dz = rd.z;
    const double A = dx * dx + dy * dy + dz * dz;
    const double B = 2 * (ox * dx + oy * dy + oz * dz);
    const double C = (ox * ox + oy * oy + oz * oz) - c.w * c.w;  // m_radius * m_radius is a float product
    double nearT, farT;
    if (!solve_quadratic_double(A, B, C, nearT, farT)) return false;
    if (!(nearT <= maxt && farT >= mint)) return false;
    if (nearT < mint) {
        if (farT > maxt) return false;
        t = (float)farT;
    } else {
        t = (float)nearT;
    }
    return true;
}
// the spheres after the triangles: a sphere wins only with a strictly smaller t (its primitive number is larger)
template <bool ANY>
D void sphere_pass(const DevScene &S, F3 o, F3 d, float mint, float maxt, Hit &best) {
    for (int k = 0; k < S.n_spheres; ++k) {
        float ts;
        if (sphere_hit(S.spheres[4 * k], o, d, mint, best.prim >= 0 ? fminf(maxt, best.t) : maxt, ts) && (best.prim < 0 || ts < best.t)) {
            best.t = ts; best.u = 0; best.v = 0; best.prim = S.n_tris + k;
            if (ANY) return;
        }
    }
}

// ---- analytic disks and cylinders (ppg_set_shapes) ----
// Transform::operator()(Point) / (Vector) of an affine 3x4 whose rows are R[0..2] (transform.h:128-137, 175-183)
D F3 aff_point(const float4 *R, F3 p) {
    return f3(R[0].x * p.x + R[0].y * p.y + R[0].z * p.z + R[0].w, R[1].x * p.x + R[1].y * p.y + R[1].z * p.z + R[1].w,
              R[2].x * p.x + R[2].y * p.y + R[2].z * p.z + R[2].w);
}
D F3 aff_vec(const float4 *R, F3 v) {
    return f3(R[0].x * v.x + R[0].y * v.y + R[0].z * v.z, R[1].x * v.x + R[1].y * v.y + R[1].z * v.z, R[2].x * v.x + R[2].y * v.y + R[2].z * v.z);
}
// Transform::operator()(Normal) (transform.h:186-197): the transposed inverse, whose rows are Rinv[0..2]
D F3 aff_normal(const float4 *Rinv, F3 n) {
    return f3(Rinv[0].x * n.x + Rinv[1].x * n.y + Rinv[2].x * n.z, Rinv[0].y * n.x + Rinv[1].y * n.y + Rinv[2].y * n.z,
              Rinv[0].z * n.x + Rinv[1].z * n.y + Rinv[2].z * n.z);
}
// Disk::rayIntersect (disk.cpp:139-162) and Cylinder::rayIntersect (cylinder.cpp:128-165; ANY: the form without t, :167-199, whose
// range tests are not NaN-aware).  The ray goes to object space through the float inverse, mint and maxt as they stand.
template <bool ANY>
D bool shape_hit(const float4 *Q, F3 o, F3 d, float mint, float maxt, float &t) {
    const F3 lo = aff_point(Q + 3, o), ld = aff_vec(Q + 3, d);
    const float4 q6 = Q[6];
    if (__float_as_int(q6.w) == PPG_SHAPE_DISK) {
        const float hit = -lo.z / ld.z;
        if (!(hit >= mint && hit <= maxt)) return false;
        const float lx = lo.x + ld.x * hit, ly = lo.y + ld.y * hit;
        if (!(lx * lx + ly * ly <= 1)) return false;
        t = hit;
        return true;
    }
    const double ox = lo.x, oy = lo.y, dx = ld.x, dy = ld.y;
    const double A = dx * dx + dy * dy;
    const double B = 2 * (dx * ox + dy * oy);
    const double C = ox * ox + oy * oy - q6.x * q6.x;  // m_radius * m_radius is a float product
    double nearT, farT;
    if (!solve_quadratic_double(A, B, C, nearT, farT)) return false;
    if (ANY) { if (nearT > maxt || farT < mint) return false; }
    else if (!(nearT <= maxt && farT >= mint)) return false;
    const double zPosNear = lo.z + ld.z * nearT;
    const double zPosFar = lo.z + ld.z * farT;
    if (zPosNear >= 0 && zPosNear <= q6.y && nearT >= mint) {
        t = (float)nearT;
    } else if (zPosFar >= 0 && zPosFar <= q6.y) {
        if (farT > maxt) return false;
        t = (float)farT;
    } else {
        return false;
    }
    return true;
}
// the shapes after the triangles and the spheres: a shape wins only with a strictly smaller t (its primitive number is larger)
template <bool ANY>
D void shape_pass(const DevScene &S, F3 o, F3 d, float mint, float maxt, Hit &best) {
    for (int k = 0; k < S.n_shapes; ++k) {
        float ts;
        if (shape_hit<ANY>(S.shapes + PPG_SHAPE_STRIDE * k, o, d, mint, best.prim >= 0 ? fminf(maxt, best.t) : maxt, ts) && (best.prim < 0 || ts < best.t)) {
            best.t = ts; best.u = 0; best.v = 0; best.prim = S.n_tris + S.n_spheres + k;
            if (ANY) return;
        }
    }
}

// The four children of a node after the slab tests, nearest first, WITHOUT indexed local arrays (a dynamically indexed array lives in
// scratch memory: the insertion sort that stood here cost k_trace 120 B of scratch traffic per lane and step).  Children that were
// missed carry t = +inf and sort to the end; a 5-comparator network on registers.  Equal distances may swap — the closest hit does not
// depend on the visiting order (ties are broken by (t, original triangle index)).
#define PPG_CSWAP(ta, ca, tb, cb) { const bool sw_ = (ta) > (tb); const float t0_ = sw_ ? (tb) : (ta), t1_ = sw_ ? (ta) : (tb); \
                                    const int c0_ = sw_ ? (cb) : (ca), c1_ = sw_ ? (ca) : (cb); ta = t0_; tb = t1_; ca = c0_; cb = c1_; }
struct Bvh4Hits { int c0, c1, c2, c3, m; };
// Slab tests of a node's four child boxes.  The traversal is bound by VALU issue slots (k_trace: 73 % of all SIMD cycles issue a vector
// instruction, profiles/r03_pmc_wait_cycles.json), and decoding the boxes to world space first — 24 x (convert, scale, add origin), then
// 24 x (subtract ray origin, multiply) — was half of a node step.  Instead the RAY is taken to the node's grid: the cell sizes are powers
// of two, so  o' = (o - origin) / cell  and  1/d' = (1/d) * cell  are exact scalings, and a plane distance is
//     t = (q - o') * (1/d')                  q = the plane's byte
// — one convert, one subtract and one multiply per plane, the two planes of an axis in one packed instruction each (v_pk_add_f32 /
// v_pk_mul_f32).  Which plane of an axis is the near one follows from the sign of 1/d: selected once per axis and node on the packed
// bytes instead of min / max per child.  Against the exact plane  origin + q * cell  the computed t carries the rounding of (o - origin)
// — a shift of at most 2^-24 |o - origin| along that axis, which matters only where it is not small against the plane distance, i.e. for
// ray origins within the node's own extent: 6e-8 of the node's size, 3 % of the builder's box padding — and two further roundings, covered by
// the factor on the exit distance as before.  The builder checks the exact planes (in double) as well as the float decode that
// trace_closest4_wave still uses.
typedef float ppg_v2f __attribute__((ext_vector_type(2)));
D Bvh4Hits bvh4_children(const Bvh4QNode *node, F3 o, F3 id, float mint, float tlim) {
    const uint4 *q = reinterpret_cast<const uint4 *>(node);
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
    const unsigned int ex = a.w & 255u, ey = (a.w >> 8) & 255u, ez = (a.w >> 16) & 255u;  // 64..154 (BvhBuilder::quantise): no overflow below
    const float osx = (o.x - __uint_as_float(a.x)) * __uint_as_float((254u - ex) << 23), idx = id.x * __uint_as_float(ex << 23);
    const float osy = (o.y - __uint_as_float(a.y)) * __uint_as_float((254u - ey) << 23), idy = id.y * __uint_as_float(ey << 23);
    const float osz = (o.z - __uint_as_float(a.z)) * __uint_as_float((254u - ez) << 23), idz = id.z * __uint_as_float(ez << 23);
    const bool nx = id.x < 0, ny = id.y < 0, nz = id.z < 0;  // (1/d is never -0, NaN or infinite: safe_inv)
    const unsigned int nearx = nx ? b.w : b.x, farx = nx ? b.x : b.w;
    const unsigned int neary = ny ? c.x : b.y, fary = ny ? b.y : c.x;
    const unsigned int nearz = nz ? c.y : b.z, farz = nz ? b.z : c.y;
    const int chs[4] = {(int)c.z, (int)c.w, (int)d.x, (int)d.y};
    float ts[4];
    int m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ppg_v2f px = {(float)((nearx >> (8 * k)) & 255u), (float)((farx >> (8 * k)) & 255u)};
        ppg_v2f py = {(float)((neary >> (8 * k)) & 255u), (float)((fary >> (8 * k)) & 255u)};
        ppg_v2f pz = {(float)((nearz >> (8 * k)) & 255u), (float)((farz >> (8 * k)) & 255u)};
        px = (px - osx) * idx; py = (py - osy) * idy; pz = (pz - osz) * idz;
        const float n = fmaxf(fmaxf(px.x, py.x), fmaxf(pz.x, mint));
        // exit distance widened by 1 + 2 gamma_3: the test stays conservative whatever the box padding
        const float f = fminf(fminf(fminf(px.y, py.y), pz.y) * 1.0000008f, tlim);
        const bool hit = (n <= f) && chs[k] != PPG_BVH4_EMPTY;
        ts[k] = hit ? n : __builtin_inff();
        m += hit ? 1 : 0;
    }
    float t0 = ts[0], t1 = ts[1], t2 = ts[2], t3 = ts[3];
    int c0 = chs[0], c1 = chs[1], c2 = chs[2], c3 = chs[3];
    PPG_CSWAP(t0, c0, t1, c1) PPG_CSWAP(t2, c2, t3, c3) PPG_CSWAP(t0, c0, t2, c2) PPG_CSWAP(t1, c1, t3, c3) PPG_CSWAP(t1, c1, t2, c2)
    Bvh4Hits r; r.c0 = c0; r.c1 = c1; r.c2 = c2; r.c3 = c3; r.m = m;
    return r;
}

// (ray, triangle)-PAIR compaction of a wave's leaf phase (k_trace).  When the leaf vote passes, some 16 – 30 lanes of the wave hold a leaf
// of 1 – 8 triangles; tested lane by lane the wave runs the triangle test max(cnt) times for a quarter of its lanes.  Here the wave lists
// its (lane, k-th triangle of that lane's leaf) pairs, deals them to ALL its lanes — a lane fetches the owner's ray with ds_bpermute —
// and runs the test once per 64 pairs.  A pair's result goes to its owner through an LDS minimum on the 64-bit key (bits of t, original
// index): the order of tri_hit's callers' update rule  t < best.t || (t == best.t && orig < bestOrig)  for t >= 0, so the closest hit is
// the same bit for bit (every pair is tested against the owner's bound at the time of the vote instead of a bound shrinking inside the
// leaf: that only admits candidates which lose the minimum).  Wave-synchronous: must be called by all 64 lanes, converged.
struct PairLds {
    unsigned long long key[64];  // per owner lane: the best (t, orig) so far
    float2 uv[64];               // ... and its barycentrics / leaf-order triangle index, written by the lane that holds the minimum
    int prim[64];
    unsigned char map[512];      // pair -> owner lane
};
// exclusive prefix sum and total of cnt (0..8) over the wave: four ballots
D void pair_prefix(int cnt, unsigned int &off, unsigned int &total) {
    off = 0; total = 0;
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) {
        const unsigned long long m = __ballot((cnt >> bit) & 1);
        off += __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u)) << bit;
        total += (unsigned int)__popcll(m) << bit;
    }
}
// cnt = this lane's triangles (0 = it holds no leaf), off / total = pair_prefix(cnt)
D void leaf_pairs(PairLds *W, const float4 *accel, int first, int cnt, unsigned int off, unsigned int total, F3 o, F3 d, float mint, float tmax, Hit &best,
                  int &bestOrig) {
    const int lane = threadIdx.x & 63;
    const bool isLeaf = cnt > 0;
    const unsigned long long own = ((unsigned long long)__float_as_uint(best.t) << 32) | (unsigned int)bestOrig;
    for (int k = 0; k < cnt; ++k) W->map[off + k] = (unsigned char)lane;
    if (isLeaf) W->key[lane] = own;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (unsigned int base = 0; base < total; base += 64) {  // (uniform)
        const unsigned int p = base + lane;
        const bool mine = p < total;
        const int src = mine ? (int)W->map[p] : lane;
        const int k = (int)(p - __shfl(off, src));
        const F3 os = f3(__shfl(o.x, src), __shfl(o.y, src), __shfl(o.z, src));
        const F3 dsv = f3(__shfl(d.x, src), __shfl(d.y, src), __shfl(d.z, src));
        const float mint_s = __shfl(mint, src), tmax_s = __shfl(tmax, src);
        const int q = __shfl(first, src) + k;
        float tt = 0, uu = 0, vv = 0;
        int orig = 0;
        const bool hit = mine && tri_hit(accel + 3 * q, os, dsv, mint_s, tmax_s, tt, uu, vv, orig);
        const unsigned long long key = ((unsigned long long)__float_as_uint(tt) << 32) | (unsigned int)orig;
        if (hit) atomicMin(&W->key[src], key);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (hit && W->key[src] == key) { W->uv[src] = make_float2(uu, vv); W->prim[src] = q; }  // (keys are unique: a triangle is in one leaf)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (isLeaf) {
        const unsigned long long kk = W->key[lane];
        if (kk != own) {
            const float2 uv = W->uv[lane];
            best.t = __uint_as_float((unsigned int)(kk >> 32)); best.u = uv.x; best.v = uv.y; best.prim = W->prim[lane];
            bestOrig = (int)(unsigned int)kk;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Closest hit by (t, original primitive index) through the BVH4 — equals brute force (conservative culling).
// ANY: return at the first triangle hit (shadow rays; only prim >= 0 is meaningful then).
// VOTE: lanes holding a leaf wait until PPG_LEAF_VOTE_TAIL lanes of the wave do (or none has an interior node left) — for callers
// whose whole wave traverses at once (k_tail); lanes that are done have left the loop and do not count.
template <bool ANY = false, bool SPH = false, bool VOTE = false>
D Hit trace_closest4(const DevScene &S, int *lds_stack_col, int stride, F3 o, F3 d, float mint, float maxt) {
    Hit best;
    best.t = __builtin_inff(); best.u = 0; best.v = 0; best.prim = -1;
    int bestOrig = 0x7fffffff;
    const F3 id = f3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    TStack st;
    int st_over[PPG_STACK_OVER];
    st.over = st_over;
    st.lds = lds_stack_col; st.stride = stride; st.sp = 0; st.cap = PPG_LDS_STACK;
    int cur = 0;
    for (;;) {  // one step per iteration: an interior node or a leaf popped from the stack (see trace_slice_bvh4)
        bool doLeaves = true;
        if (VOTE) {
            const unsigned long long leafLanes = __ballot(cur < 0), nodeLanes = __ballot(cur >= 0);
            doLeaves = __popcll(leafLanes) >= PPG_LEAF_VOTE_TAIL || nodeLanes == 0ull;
        }
        if (cur >= 0) {
            const Bvh4Hits hc = bvh4_children(S.bvh4 + cur, o, id, mint, fminf(maxt, best.t));
            if (hc.m > 0) {
                st.push_children(hc.m, hc.c1, hc.c2, hc.c3);
                cur = hc.c0;
            } else {
                if (st.sp == 0) break;
                cur = st.pop();
            }
        } else if (doLeaves) {
            const int code = ~cur;
            const int first = code >> 3, cnt = (code & 7) + 1;
            for (int q = first; q < first + cnt; ++q) {
                float tt, uu, vv;
                const float4 *T = S.accel + 3 * q;
                int orig;
                if (tri_hit(T, o, d, mint, fminf(maxt, best.t), tt, uu, vv, orig)) {
                    if (ANY) { best.t = tt; best.prim = q; return best; }
                    if (tt < best.t || (tt == best.t && orig < bestOrig)) { best.t = tt; best.u = uu; best.v = vv; best.prim = q; bestOrig = orig; }
                }
            }
            if (st.sp == 0) break;
            cur = st.pop();
        }
    }
    if (SPH && S.n_spheres) sphere_pass<ANY>(S, o, d, mint, maxt, best);
    if (PPG_SHAPES && SPH && S.n_shapes && !(ANY && best.prim >= 0)) shape_pass<ANY>(S, o, d, mint, maxt, best);
    return best;
}

#ifndef PPG_PAIR_VOTE
#define PPG_PAIR_VOTE 32       // k_trace: the leaf phase runs when the wave's leaves hold this many triangles (or no lane has an interior node)
#endif
// trace_closest4<false, SPH, VOTE> that can be SUSPENDED (k_tail's crowd phase).  A wave's lanes trace one ray each and the lengths of
// the traversals differ by an order of magnitude: without this the wave waits for its longest ray with most lanes idle.  When no more than
// `suspend_lanes` lanes are still traversing (of more than twice as many that began), they park their state — node / leaf at hand, stack
// pointer, original index of the best hit in `park`, the best hit in `best`, the stack where it is, in the lane's LDS column — and return
// false; the caller shades the other lanes' hits and calls again with resume = true together with those lanes' next rays: a long ray spans
// several rounds of the wave instead of holding one up.  A lane whose stack has overflowed into its private array is waited for (rare).
// The closest hit is the same bit for bit: the traversal is the same, only interleaved differently with other lanes' work.
#ifndef PPG_TAIL_SUSPEND
#define PPG_TAIL_SUSPEND 8
#endif
template <bool SPH>
D bool trace_closest4_resume(const DevScene &S, int *lds_stack_col, int stride, F3 o, F3 d, float mint, float maxt, bool resume, int *park, int pstride,
                             Hit &best, int suspend_lanes) {
    int bestOrig = 0x7fffffff, cur = 0;
    const F3 id = f3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    TStack st;
    int st_over[PPG_STACK_OVER];
    st.over = st_over;
    st.lds = lds_stack_col; st.stride = stride; st.sp = 0; st.cap = PPG_LDS_STACK;
    if (resume) { cur = park[0]; st.sp = park[pstride]; bestOrig = park[2 * pstride]; }
    else { best.t = __builtin_inff(); best.u = 0; best.v = 0; best.prim = -1; }
    const int n0 = (int)__popcll(__ballot(true));
    for (;;) {
        const unsigned long long leafLanes = __ballot(cur < 0), nodeLanes = __ballot(cur >= 0);
        if (suspend_lanes && n0 > 2 * suspend_lanes && (int)__popcll(leafLanes | nodeLanes) <= suspend_lanes && __ballot(st.sp > PPG_LDS_STACK) == 0ull) {
            park[0] = cur; park[pstride] = st.sp; park[2 * pstride] = bestOrig;
            return false;
        }
        const bool doLeaves = __popcll(leafLanes) >= PPG_LEAF_VOTE_TAIL || nodeLanes == 0ull;
        if (cur >= 0) {
            const Bvh4Hits hc = bvh4_children(S.bvh4 + cur, o, id, mint, fminf(maxt, best.t));
            if (hc.m > 0) {
                st.push_children(hc.m, hc.c1, hc.c2, hc.c3);
                cur = hc.c0;
            } else {
                if (st.sp == 0) break;
                cur = st.pop();
            }
        } else if (doLeaves) {
            const int code = ~cur;
            const int first = code >> 3, cnt = (code & 7) + 1;
            for (int q = first; q < first + cnt; ++q) {
                float tt, uu, vv;
                int orig;
                if (tri_hit(S.accel + 3 * q, o, d, mint, fminf(maxt, best.t), tt, uu, vv, orig)) {
                    if (tt < best.t || (tt == best.t && orig < bestOrig)) { best.t = tt; best.u = uu; best.v = vv; best.prim = q; bestOrig = orig; }
                }
            }
            if (st.sp == 0) break;
            cur = st.pop();
        }
    }
    if (SPH && S.n_spheres) sphere_pass<false>(S, o, d, mint, maxt, best);
    if (PPG_SHAPES && SPH && S.n_shapes) shape_pass<false>(S, o, d, mint, maxt, best);
    return true;
}

// ONE ray traversed by a whole WAVE (k_tail, when a wave carries only a handful of live paths).  A lone lane's traversal is a chain of
// ~17 dependent node / leaf fetches, almost every one an L2 miss (the BVH and the triangle records are 70 MB against 4 MB of L2 per XCD):
// measured 36 k cycles of a lone path's 54 k-cycle bounce.  Here the wave works on up to 16 stack entries at once — four lanes
// per entry, one child box or one triangle each — so the dependent chain is as long as the tree is deep, not as the traversal is long,
// and all fetches of a level are in flight together.  Entries are node indices / leaf codes on a wave-wide stack laid over the wave's 64
// LDS stack columns (entry k = row k / 64, column k % 64).  No front-to-back order is kept: more nodes are visited than by the ordered
// per-lane walk, which costs nothing in a wave that would otherwise idle.  Same box arithmetic, same triangle test, same (t, original
// index) minimum as trace_closest4, so the hit is the same bit for bit.  Must be called by all 64 lanes with identical arguments.
#ifndef PPG_COOP_MAX
#define PPG_COOP_MAX 16  // live lanes of a wave up to which k_tail traces cooperatively (measured per-iteration cycles, §7: 1 lane 36 k per-lane vs ~14 k).
                         // 6 until round 6; with the suspended traversals (which need more than 2 x PPG_TAIL_SUSPEND lanes) 10 and 16 measured +0.7 / +0.9 %
#endif
// ROWS: the rows of 64 entries the wave-wide stack may use (ppg_debug_intersect_mode runs it with 1 as well, to reach the overrun)
template <int ROWS = PPG_LDS_STACK>
D Hit trace_closest4_wave(const DevScene &S, int *wave_stack /* this wave's column 0 */, int stride, F3 o, F3 d, float mint, float maxt,
                          int *probe_steps = nullptr) {
    const int lane = threadIdx.x & 63, g = lane >> 2, c = lane & 3;
    Hit best;
    best.t = __builtin_inff(); best.u = 0; best.v = 0; best.prim = -1;
    int bestOrig = 0x7fffffff;
    const F3 id = f3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    auto slot = [&](int k) -> int & { return wave_stack[(k >> 6) * stride + (k & 63)]; };
    int count = 1;
    if (S.n_top > 0) {
        // first step: the tree's top cut — up to 64 subtrees that partition the scene, each with the box its parent's node would decode for
        // it — tested by one lane each, instead of the first three levels one dependent step after the other
        int push = PPG_BVH4_EMPTY;
        if (lane < S.n_top) {
            float4 lo = S.bvh_top[2 * lane], hi = S.bvh_top[2 * lane + 1];
            PPG_PIN4(lo); PPG_PIN4(hi);
            const float ax = (lo.x - o.x) * id.x, bx = (hi.x - o.x) * id.x;
            const float ay = (lo.y - o.y) * id.y, by = (hi.y - o.y) * id.y;
            const float az = (lo.z - o.z) * id.z, bz = (hi.z - o.z) * id.z;
            const float n = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), mint));
            const float f = fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.0000008f, maxt);
            if (n <= f) push = __float_as_int(lo.w);
        }
        const unsigned long long pm = __ballot(push != PPG_BVH4_EMPTY);
        if (push != PPG_BVH4_EMPTY) slot((int)__popcll(pm & ((1ull << lane) - 1ull))) = push;
        count = (int)__popcll(pm);
    } else if (lane == 0) slot(0) = 0;
    for (;;) {
        if (count == 0) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the entries other lanes pushed in the previous step (LDS, wave-synchronous)
        const int take = count < 16 ? count : 16, base = count - take;
        if (probe_steps) ++*probe_steps;
        const int entry = g < take ? slot(base + g) : PPG_BVH4_EMPTY;
        count = base;
        const float tlim = fminf(maxt, best.t);
        int push = PPG_BVH4_EMPTY;
        float tt = __builtin_inff(), uu = 0, vv = 0;
        int tq = -1, torig = 0x7fffffff;
        // A step is ONE memory round trip for the whole wave: every lane issues all the loads of its entry — the node's four 16-byte words,
        // or its triangle's three — back to back and waits once (PPG_PIN).  Left to itself the compiler sinks each load to its first use
        // behind the early-outs of the tests, which made a triangle four dependent round trips (projection axis, t, barycentrics, original
        // index) and a node up to three: a lone path's traversal, a chain of such steps, spent 2100 cycles per step (cycle probe).
        if (entry >= 0 && entry != PPG_BVH4_EMPTY) {  // interior node: this lane tests child c (the arithmetic of bvh4q_load / bvh4_children)
            const uint4 *q = reinterpret_cast<const uint4 *>(S.bvh4 + entry);
            uint4 a = q[0], b = q[1], cc = q[2], dd = q[3];
            PPG_PIN4(a); PPG_PIN4(b); PPG_PIN4(cc); PPG_PIN4(dd);
            const float ox = __uint_as_float(a.x), oy = __uint_as_float(a.y), oz = __uint_as_float(a.z);
            const float sx = __uint_as_float((a.w & 255u) << 23), sy = __uint_as_float(((a.w >> 8) & 255u) << 23), sz = __uint_as_float(((a.w >> 16) & 255u) << 23);
            const int sh = 8 * c;
            const float lx = ox + (float)((b.x >> sh) & 255u) * sx, ly = oy + (float)((b.y >> sh) & 255u) * sy, lz = oz + (float)((b.z >> sh) & 255u) * sz;
            const float hx = ox + (float)((b.w >> sh) & 255u) * sx, hy = oy + (float)((cc.x >> sh) & 255u) * sy, hz = oz + (float)((cc.y >> sh) & 255u) * sz;
            const int ch = c == 0 ? (int)cc.z : (c == 1 ? (int)cc.w : (c == 2 ? (int)dd.x : (int)dd.y));
            const float ax = (lx - o.x) * id.x, bx = (hx - o.x) * id.x;
            const float ay = (ly - o.y) * id.y, by = (hy - o.y) * id.y;
            const float az = (lz - o.z) * id.z, bz = (hz - o.z) * id.z;
            const float n = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), mint));
            const float f = fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.0000008f, tlim);
            if (n <= f && ch != PPG_BVH4_EMPTY) push = ch;
        } else if (entry != PPG_BVH4_EMPTY) {  // leaf: this lane tests triangle c (and c + 4 of a leaf of more than four)
            const int code = ~entry, first = code >> 3, cnt = (code & 7) + 1;
            for (int k = c; k < cnt; k += 4) {
                const float4 *T = S.accel + 3 * (first + k);
                float t1, u1, v1;
                int orig;
                if (tri_hit(T, o, d, mint, tlim, t1, u1, v1, orig)) {
                    if (t1 < tt || (t1 == tt && orig < torig)) { tt = t1; uu = u1; vv = v1; tq = first + k; torig = orig; }
                }
            }
        }
        // children that were hit go onto the stack (any order).  The stack is ROWS (PPG_LDS_STACK) rows of 64: a traversal that would overrun it
        // (never observed in a render; heavily overlapping boxes could) is abandoned — prim = -2 — and the caller walks that ray with one lane
        // instead (tests/test_traversal_gpu.py takes that way with a stack of one row).
        const unsigned long long pm = __ballot(push != PPG_BVH4_EMPTY);
        if (count + (int)__popcll(pm) > ROWS * 64) { best.prim = -2; return best; }
        if (push != PPG_BVH4_EMPTY) slot(count + (int)__popcll(pm & ((1ull << lane) - 1ull))) = push;
        count += (int)__popcll(pm);
        // the triangle hits of this step, folded into the closest hit so far by (t, original index): a step rarely has more than one, so
        // the lanes that hit are read one after the other (v_readlane, no LDS round trips) instead of two 64-lane shuffle reductions
        for (unsigned long long hm = __ballot(tq >= 0); hm; hm &= hm - 1ull) {
            const int src = __ffsll((long long)hm) - 1;
            const float ts = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tt), src));
            const int os = __builtin_amdgcn_readlane(torig, src);
            if (ts < best.t || (ts == best.t && os < bestOrig)) {
                best.t = ts; bestOrig = os;
                best.u = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uu), src));
                best.v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vv), src));
                best.prim = __builtin_amdgcn_readlane(tq, src);
            }
        }
    }
    if (S.n_spheres) sphere_pass<false>(S, o, d, mint, maxt, best);
    if (PPG_SHAPES && S.n_shapes) shape_pass<false>(S, o, d, mint, maxt, best);
    return best;
}

// Intersection record: fillIntersectionRecord (skdtree.h:343-430) + computeShadingFrame (util.cpp:603-608)
struct Isect {
    F3 p, geoN, s, t, n, wi;
    int material, emitter;
};
D F3 to_local(const Isect &I, F3 v) { return f3(dot3(v, I.s), dot3(v, I.t), dot3(v, I.n)); }
D F3 to_world(const Isect &I, F3 v) { return I.s * v.x + I.t * v.y + I.n * v.z; }

// Sphere::fillIntersectionRecord (sphere.cpp:213-263): position re-projected onto the sphere, its normal, dpdu of the (theta, phi)
// parameterisation as the tangent; worldToObject of a vector taken as the transposed rotation.  `o` = the ray origin.
D void fill_isect_sphere(const DevScene &S, const Hit &h, F3 o, F3 d, Isect &I) {
    const float4 *Q = S.spheres + 4 * (h.prim - S.n_tris);
    const float4 c4 = Q[0], r0 = Q[1], r1 = Q[2], r2 = Q[3];
    const F3 c = f3(c4.x, c4.y, c4.z);
    F3 p = o + d * h.t;
    p = c + norm3(p - c) * c4.w;
    const F3 v = p - c;
    const F3 local = f3(r0.x * v.x + r1.x * v.y + r2.x * v.z, r0.y * v.x + r1.y * v.y + r2.y * v.z, r0.z * v.x + r1.z * v.y + r2.z * v.z);
    const F3 du = f3(-local.y, local.x, 0.0f) * (2 * PPG_PI_F);
    const F3 dpdu = f3(r0.x * du.x + r0.y * du.y + r0.z * du.z, r1.x * du.x + r1.y * du.y + r1.z * du.z, r2.x * du.x + r2.y * du.y + r2.z * du.z);
    F3 n = norm3(p - c);
    if (__float_as_int(r2.w)) n = n * -1.0f;
    I.p = p; I.geoN = n; I.n = n;
    I.s = norm3(dpdu - n * dot3(n, dpdu));
    I.t = cross3(n, I.s);
    I.wi = to_local(I, -d);
    I.material = __float_as_int(r0.w);
    I.emitter = __float_as_int(r1.w);
}
// Disk::fillIntersectionRecord (disk.cpp:169-198) and Cylinder::fillIntersectionRecord (cylinder.cpp:201-230), then computeShadingFrame(n,
// dpdu).  The disk's local hit point is what its ray test kept in `temp`: the same arithmetic again.  Its geometric normal is its shading
// normal (the reference leaves its.geoFrame unset there: DESIGN.md).  `o` = the ray origin.
D void fill_isect_shape(const DevScene &S, const Hit &h, F3 o, F3 d, Isect &I) {
    const float4 *Q = S.shapes + PPG_SHAPE_STRIDE * (h.prim - S.n_tris - S.n_spheres);
    const float4 q6 = Q[6], q7 = Q[7];
    F3 p = o + d * h.t, n, dpdu;
    if (__float_as_int(q6.w) == PPG_SHAPE_DISK) {
        const F3 lo = aff_point(Q + 3, o), ld = aff_vec(Q + 3, d);
        const float lx = lo.x + ld.x * h.t, ly = lo.y + ld.y * h.t;
        const float r = __builtin_sqrtf(lx * lx + ly * ly), invR = (r == 0) ? 0.0f : (1.0f / r);
        dpdu = aff_vec(Q, r != 0 ? f3(lx * invR, ly * invR, 0.0f) : f3(1.0f, 0.0f, 0.0f));
        n = norm3(aff_normal(Q + 3, f3(0.0f, 0.0f, 1.0f)));
    } else {
        const F3 local = aff_point(Q + 3, p);
        dpdu = aff_vec(Q, f3(-local.y, local.x, 0.0f) * (2 * PPG_PI_F));
        const F3 dpdv = aff_vec(Q, f3(0.0f, 0.0f, q6.y));
        n = cross3(norm3(dpdu), norm3(dpdv));
        p = p + n * (q6.x - __builtin_sqrtf(local.x * local.x + local.y * local.y));
    }
    if (__float_as_int(q7.z)) n = n * -1.0f;
    I.p = p; I.geoN = n; I.n = n;
    I.s = norm3(dpdu - n * dot3(n, dpdu));
    I.t = cross3(n, I.s);
    I.wi = to_local(I, -d);
    I.material = __float_as_int(q7.x);
    I.emitter = __float_as_int(q7.y);
}
// a hit that is not a triangle: sphere or shape
D void fill_isect_analytic(const DevScene &S, const Hit &h, F3 o, F3 d, Isect &I) {
    if (PPG_SHAPES && h.prim >= S.n_tris + S.n_spheres) fill_isect_shape(S, h, o, d, I);
    else fill_isect_sphere(S, h, o, d, I);
}
D void fill_isect(const DevScene &S, const Hit &h, F3 d, Isect &I) {
    const float4 *T = S.tris + 3 * h.prim;
    float4 q0 = T[0], q1 = T[1];
    F3 p0 = f3(q0.x, q0.y, q0.z), p1 = f3(q1.x, q1.y, q1.z), p2 = ld3(T + 2);
    F3 b = f3(1 - h.u - h.v, h.u, h.v);
    I.p = p0 * b.x + p1 * b.y + p2 * b.z;
    F3 side1 = p1 - p0, side2 = p2 - p0;
    F3 fn = cross3(side1, side2);
    float len = len3(fn);
    if (!(fn.x == 0 && fn.y == 0 && fn.z == 0)) fn = div3(fn, len);
    F3 shN;
    if (S.normals) {
        const float4 *Nn = S.normals + 3 * h.prim;
        shN = norm3(ld3(Nn) * b.x + ld3(Nn + 1) * b.y + ld3(Nn + 2) * b.z);
        if (dot3(fn, shN) < 0) fn = -fn;
    } else {
        shN = fn;
    }
    I.geoN = fn;
    I.n = shN;
    I.s = norm3(side1 - shN * dot3(shN, side1));
    I.t = cross3(shN, I.s);
    I.wi = to_local(I, -d);
    I.material = __float_as_int(q0.w);
    I.emitter = __float_as_int(q1.w);
}

// ---- bitmap textures (FULL kernels; include/ppg.h ppg_texture) ----
// What a textured BSDF needs of the intersection besides the frame: its.uv, its.dpdu / dpdv, the material's texture word.
struct TexInfo {
    unsigned int tex;
    float u, v;
    F3 dpdu, dpdv;
};
// fillIntersectionRecord for a triangle whose BSDF may read a bitmap: as fill_isect, plus the texture coordinates (skdtree.h:403-410)
// and — on meshes that carry them — TriMesh::computeUVTangents' tangents (trimesh.cpp:683-735) as dpdu / dpdv (skdtree.h:374-381),
// which then also span the shading frame.  SLOTS: the material may carry a bitmap on specular / alpha / opacity (ppg_set_material_textures),
// which asks for the same as the texture word does; false where sort_slice has sent such surfaces elsewhere (MSET_COMMON).
// (the two pieces of its.uv that tex_eval_hit shares with it: a NaN row = the mesh carries no texture coordinates; the interpolation)
D bool tri_has_uvs(float2 t0, float2 t1, float2 t2) { return !(t0.x != t0.x) && !(t1.x != t1.x) && !(t2.x != t2.x); }
D void tri_uv_at(float2 t0, float2 t1, float2 t2, F3 b, float &u, float &v) {
    u = t0.x * b.x + t1.x * b.y + t2.x * b.z;
    v = t0.y * b.x + t1.y * b.y + t2.y * b.z;
}
template <bool SLOTS = true>
D void fill_isect_tex(const DevScene &S, const Hit &h, F3 d, Isect &I, TexInfo &X) {
    const float4 *T = S.tris + 3 * h.prim;
    float4 q0 = T[0], q1 = T[1];
    F3 p0 = f3(q0.x, q0.y, q0.z), p1 = f3(q1.x, q1.y, q1.z), p2 = ld3(T + 2);
    F3 b = f3(1 - h.u - h.v, h.u, h.v);
    I.p = p0 * b.x + p1 * b.y + p2 * b.z;
    F3 side1 = p1 - p0, side2 = p2 - p0;
    F3 fn = cross3(side1, side2);
    float len = len3(fn);
    const F3 nraw = fn;
    if (!(fn.x == 0 && fn.y == 0 && fn.z == 0)) fn = div3(fn, len);
    F3 shN;
    if (S.normals) {
        const float4 *Nn = S.normals + 3 * h.prim;
        shN = norm3(ld3(Nn) * b.x + ld3(Nn + 1) * b.y + ld3(Nn + 2) * b.z);
        if (dot3(fn, shN) < 0) fn = -fn;
    } else {
        shN = fn;
    }
    I.geoN = fn;
    I.n = shN;
    I.material = __float_as_int(q0.w);
    I.emitter = __float_as_int(q1.w);
    bool textured;
    if (SLOTS) {
        const float4 row = S.materials[PPG_MAT_STRIDE * (size_t)I.material + 5];
        X.tex = __float_as_uint(row.x);
        textured = (X.tex | __float_as_uint(row.y) | __float_as_uint(row.z) | __float_as_uint(row.w)) != 0u;
    } else {
        X.tex = __float_as_uint(S.materials[PPG_MAT_STRIDE * (size_t)I.material + 5].x);
        textured = X.tex != 0u;
    }
#if PPG_MFD
    if (SLOTS && S.mfd) textured = textured || (__float_as_uint(S.mfd[I.material].y) & PPG_MFDF_ANISO) != 0u;
#endif
#if PPG_BLEND
    if (SLOTS && S.blend) textured = textured || (__float_as_uint(S.blend[PPG_BLEND_STRIDE * (size_t)I.material + 3].y) & PPG_BLENDF_TEXTURED) != 0u;
#endif
    F3 dpdu = side1;
    if (textured) {
        X.u = b.y; X.v = b.z;
        X.dpdu = side1; X.dpdv = side2;
        if (S.uvs) {
            const float2 t0 = S.uvs[3 * (size_t)h.prim], t1 = S.uvs[3 * (size_t)h.prim + 1], t2 = S.uvs[3 * (size_t)h.prim + 2];
            if (tri_has_uvs(t0, t1, t2)) {
                tri_uv_at(t0, t1, t2, b, X.u, X.v);
                const float dUV1x = t1.x - t0.x, dUV1y = t1.y - t0.y, dUV2x = t2.x - t0.x, dUV2y = t2.y - t0.y;
                if (len != 0) {
                    const float determinant = dUV1x * dUV2y - dUV1y * dUV2x;
                    if (determinant == 0) {
                        const F3 a = div3(nraw, len);  // coordinateSystem(n / length, dpdu, dpdv), util.cpp:592-601
                        if (ppg_abs(a.x) > ppg_abs(a.y)) {
                            float invLen = 1.0f / __builtin_sqrtf(a.x * a.x + a.z * a.z);
                            X.dpdv = f3(a.z * invLen, 0.0f, -a.x * invLen);
                        } else {
                            float invLen = 1.0f / __builtin_sqrtf(a.y * a.y + a.z * a.z);
                            X.dpdv = f3(0.0f, a.z * invLen, -a.y * invLen);
                        }
                        X.dpdu = cross3(X.dpdv, a);
                    } else {
                        const float invDet = 1.0f / determinant;
                        X.dpdu = (side1 * dUV2y - side2 * dUV1y) * invDet;
                        X.dpdv = (side1 * -dUV2x + side2 * dUV1x) * invDet;
                    }
                }
            }
        }
        dpdu = X.dpdu;
    }
    I.s = norm3(dpdu - shN * dot3(shN, dpdu));
    I.t = cross3(shN, I.s);
    I.wi = to_local(I, -d);
}

D int tex_modulo(int a, int b) { int r = a % b; return (r < 0) ? r + b : r; }  // math.h:67-70
// MIPMap::evalTexel (mipmap.h:503-563) on level 0
D F3 tex_texel(const DevTex &t, int x, int y) {
    if (x < 0 || x >= t.w) {
        switch (t.wrap_u) {
            case PPG_WRAP_REPEAT: x = tex_modulo(x, t.w); break;
            case PPG_WRAP_CLAMP: x = x < 0 ? 0 : t.w - 1; break;
            case PPG_WRAP_MIRROR: x = tex_modulo(x, 2 * t.w); if (x >= t.w) x = 2 * t.w - x - 1; break;
            case PPG_WRAP_ZERO: return f3s(0.0f);
            default: return f3s(1.0f);
        }
    }
    if (y < 0 || y >= t.h) {
        switch (t.wrap_v) {
            case PPG_WRAP_REPEAT: y = tex_modulo(y, t.h); break;
            case PPG_WRAP_CLAMP: y = y < 0 ? 0 : t.h - 1; break;
            case PPG_WRAP_MIRROR: y = tex_modulo(y, 2 * t.h); if (y >= t.h) y = 2 * t.h - y - 1; break;
            case PPG_WRAP_ZERO: return f3s(0.0f);
            default: return f3s(1.0f);
        }
    }
    const float4 v = t.texels[(size_t)y * t.w + x];
    return f3(v.x, v.y, v.z);
}
// Texture2D::eval(its) without UV partials (texture.cpp:112-121) → BitmapTexture::eval(uv) (bitmap.cpp:431-452)
D F3 tex_eval(const DevTex &t, float iu, float iv) {
    const float ux = iu * t.su + t.ou, uy = iv * t.sv + t.ov;
    if (t.nearest) return tex_texel(t, (int)__builtin_floorf(ux * t.w), (int)__builtin_floorf(uy * t.h));
    if (!ppg_isfinite(ux) || !ppg_isfinite(uy)) return f3s(0.0f);
    const float u = ux * t.w - 0.5f, v = uy * t.h - 0.5f;
    const int xPos = (int)__builtin_floorf(u), yPos = (int)__builtin_floorf(v);
    const float dx1 = u - xPos, dx2 = 1.0f - dx1, dy1 = v - yPos, dy2 = 1.0f - dy1;
    return tex_texel(t, xPos, yPos) * dx2 * dy2 + tex_texel(t, xPos, yPos + 1) * dx2 * dy1 + tex_texel(t, xPos + 1, yPos) * dx1 * dy2 +
           tex_texel(t, xPos + 1, yPos + 1) * dx1 * dy1;
}
// Texture2D::evalGradient(its) (texture.cpp:123-131) over MIPMap::evalGradientBilinear(0, uv) (mipmap.h:601-626): luminance of d/du, d/dv
D void tex_gradient_lum(const DevTex &t, float iu, float iv, float &gu, float &gv) {
    const float ux = iu * t.su + t.ou, uy = iv * t.sv + t.ov;
    gu = 0.0f; gv = 0.0f;
    if (t.nearest || !ppg_isfinite(ux) || !ppg_isfinite(uy)) return;
    const float u = ux * t.w - 0.5f, v = uy * t.h - 0.5f;
    const int xPos = (int)__builtin_floorf(u), yPos = (int)__builtin_floorf(v);
    const float dx = u - xPos, dy = v - yPos;
    const F3 p00 = tex_texel(t, xPos, yPos), p10 = tex_texel(t, xPos + 1, yPos), p01 = tex_texel(t, xPos, yPos + 1), p11 = tex_texel(t, xPos + 1, yPos + 1);
    const F3 tmp = p01 + p10 - p11;
    F3 g0 = (p10 + p00 * (dy - 1) - tmp * dy) * (float)t.w;
    F3 g1 = (p01 + p00 * (dx - 1) - tmp * dx) * (float)t.h;
    g0 = g0 * t.su;
    g1 = g1 * t.sv;
    gu = g0.x * 0.212671f + g0.y * 0.715160f + g0.z * 0.072169f;
    gv = g1.x * 0.212671f + g1.y * 0.715160f + g1.z * 0.072169f;
}
// BumpMap::getFrame (bumpmap.cpp:135-160): the perturbed frame (s, t, n)
D void bump_frame(const DevScene &S, const Isect &I, const TexInfo &X, F3 &ps, F3 &pt, F3 &pn) {
    float dDispDu, dDispDv;
    tex_gradient_lum(S.textures[(X.tex >> 16) - 1], X.u, X.v, dDispDu, dDispDv);
    const F3 dpdu = X.dpdu + I.n * (dDispDu - dot3(I.n, X.dpdu));
    const F3 dpdv = X.dpdv + I.n * (dDispDv - dot3(I.n, X.dpdv));
    pn = norm3(cross3(dpdu, dpdv));
    ps = norm3(dpdu - pn * dot3(pn, dpdu));
    pt = cross3(pn, ps);
    if (dot3(pn, I.geoN) < 0) pn = pn * -1.0f;
}
#if PPG_NORMALMAP_NULL
static __device__ __attribute__((noinline)) float4 tex_eval_slot(const DevTex *textures, unsigned int slot, float u, float v);
// NormalMap::getFrame (normalmap.cpp:108-124): the frame (s, t, n) around the normal the RGB texel names in the unperturbed shading frame.
// Unlike bumpmap.cpp it does not flip a normal that points against the geometric one.  (A texel that decodes to the zero vector gives
// Mitsuba's NaN frame.)
D void normal_frame(const DevScene &S, const Isect &I, const TexInfo &X, F3 &ps, F3 &pt, F3 &pn) {
    const float4 c = tex_eval_slot(S.textures, X.tex >> 16, X.u, X.v);
    const F3 n = f3(2 * c.x - 1, 2 * c.y - 1, 2 * c.z - 1);
    pn = norm3(to_world(I, n));
    ps = norm3(X.dpdu - pn * dot3(pn, X.dpdu));
    pt = cross3(pn, ps);
}
#endif

// AreaLight::eval (area.cpp:104-109)
D F3 eval_Le(const DevScene &S, const Isect &I, F3 dir) {
    if (I.emitter < 0) return f3s(0.0f);
    if (dot3(I.n, dir) <= 0) return f3s(0.0f);
    float4 r = S.emitters[I.emitter];
    return f3(r.x, r.y, r.z);
}

// DiscreteDistribution::sample (pmf.h:124-136) on a normalised cdf with `entries` values (cdf[0] = 0)
D int pmf_sample(const float *cdf, int entries, float v) {
    int lo = 0, hi = entries;  // std::lower_bound: first position with cdf[pos] >= v
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (cdf[mid] < v) lo = mid + 1; else hi = mid;
    }
    int index = lo - 1;
    if (index < 0) index = 0;
    if (index > entries - 2) index = entries - 2;
    while (index < entries - 1 && cdf[index + 1] - cdf[index] == 0) ++index;
    return index;
}

// Direct illumination sample on an area emitter — Scene::sampleAttenuatedEmitterDirect (scene.cpp:876-897) up to,
// not including, the transmittance test: emitter choice, AreaLight::sampleDirect (area.cpp:158-173),
// Shape::sampleDirect (shape.cpp:102-115), TriMesh::samplePosition (trimesh.cpp:412-423), Triangle::sample
// (triangle.cpp:24-58).  Returns radiance / pdf (solid angle, before the emitter-choice probability), or zero
// with ds.pdf = 0.
struct DirectSample {
    F3 n, d;
    float dist, pdf, em_pdf;
    bool is_env;
    bool is_delta;  // point / spot / directional: discrete measure, not on a surface (no BSDF / D-tree density in the MIS weight, GP:1987-1994)
    F3 sd;        // direction and length of the shadow ray: Scene::evalTransmittance recomputes them from the two end points
    float sdist;  // (scene.cpp:621-623) — identical to (d, dist) for area emitters, a rounding apart for the environment emitter
};

D F3 cosine_hemisphere(float sx, float sy);  // defined below

// BSphere::rayIntersect (bsphere.h:88-95) + solveQuadratic (util.cpp:447-485) against the environment emitter's sphere
D bool bsphere_intersect(const DevScene &S, F3 o_, F3 d, float &nearHit, float &farHit) {
    F3 o = o_ - f3(S.bsphere.x, S.bsphere.y, S.bsphere.z);
    float A = dot3(d, d), B = 2 * dot3(o, d), Cq = dot3(o, o) - S.bsphere.w * S.bsphere.w;
    if (A == 0) {
        if (B != 0) { nearHit = farHit = -Cq / B; return true; }
        return false;
    }
    float discrim = B * B - 4.0f * A * Cq;
    if (discrim < 0) return false;
    float temp, sqrtDiscrim = __builtin_sqrtf(discrim);
    if (B < 0) temp = -0.5f * (B - sqrtDiscrim);
    else temp = -0.5f * (B + sqrtDiscrim);
    nearHit = temp / A;
    farHit = Cq / temp;
    if (nearHit > farHit) { float t = nearHit; nearHit = farHit; farHit = t; }
    return true;
}
// ConstantBackgroundEmitter::fillDirectSamplingRecord (constant.cpp:240-254): can a ray that left the scene be attributed to it?
D bool env_fill_direct(const DevScene &S, F3 o, F3 d) {
    float nearT, farT;
    return bsphere_intersect(S, o, d, nearT, farT) && !(nearT > 0) && !(farT < 0);
}
// ConstantBackgroundEmitter::pdfDirect (constant.cpp:216-231), solid angle; cos_refn = dot(d, refN), or < -1.5 when refN = 0
D float env_pdf_direct(float cos_refn) { return cos_refn < -1.5f ? PPG_INV_PI_F * 0.25f : PPG_INV_PI_F * ppg_max(0.0f, cos_refn); }
D float lum3(F3 s);  // defined below
// ---- EnvironmentMap (emitters/envmap.cpp), level-0 bilinear lookups (mipmap.h:503-596: u repeats, v clamps) ----
D F3 envmap_to_world(const DevScene &S, F3 v) {
    return f3(S.em_R[0] * v.x + S.em_R[1] * v.y + S.em_R[2] * v.z, S.em_R[3] * v.x + S.em_R[4] * v.y + S.em_R[5] * v.z, S.em_R[6] * v.x + S.em_R[7] * v.y + S.em_R[8] * v.z);
}
D F3 envmap_to_local(const DevScene &S, F3 v) {
    return f3(S.em_R[0] * v.x + S.em_R[3] * v.y + S.em_R[6] * v.z, S.em_R[1] * v.x + S.em_R[4] * v.y + S.em_R[7] * v.z, S.em_R[2] * v.x + S.em_R[5] * v.y + S.em_R[8] * v.z);
}
D F3 envmap_texel(const DevScene &S, int x, int y) {
    if (x < 0 || x >= S.em_w) { x %= S.em_w; if (x < 0) x += S.em_w; }
    if (y < 0 || y >= S.em_h) y = y < 0 ? 0 : S.em_h - 1;
    const float4 t = S.em_texels[(size_t)y * S.em_w + x];
    return f3(t.x, t.y, t.z);
}
D int envmap_clamp_row(const DevScene &S, int y) { return y < 0 ? 0 : (y > S.em_h - 1 ? S.em_h - 1 : y); }
D bool finitef(float v) { return (ppg_f2u(v) & 0x7f800000u) != 0x7f800000u; }
// evalEnvironment (envmap.cpp:381-407) of a ray without differentials travelling along the world direction d
D F3 envmap_eval(const DevScene &S, F3 dWorld) {
    const F3 v = envmap_to_local(S, dWorld);
    const float uvx = dm_atan2(v.x, -v.z) * (PPG_INV_PI_F * 0.5f), uvy = dm_acos(v.y) * PPG_INV_PI_F;
    if (!finitef(uvx) || !finitef(uvy)) return f3s(0.0f);
    const float u = uvx * S.em_w - 0.5f, vv = uvy * S.em_h - 0.5f;
    const int xPos = (int)__builtin_floorf(u), yPos = (int)__builtin_floorf(vv);
    const float dx1 = u - xPos, dx2 = 1.0f - dx1, dy1 = vv - yPos, dy2 = 1.0f - dy1;
    const F3 value = envmap_texel(S, xPos, yPos) * dx2 * dy2 + envmap_texel(S, xPos, yPos + 1) * dx2 * dy1 + envmap_texel(S, xPos + 1, yPos) * dx1 * dy2 +
                     envmap_texel(S, xPos + 1, yPos + 1) * dx1 * dy1;
    return value * S.em_scale;
}
// the radiance a ray travelling along d sees once it has left the scene: constant or image-based environment emitter
D F3 env_radiance(const DevScene &S, F3 d) { return S.env.w == 2.0f ? envmap_eval(S, d) : f3(S.env.x, S.env.y, S.env.z); }
// sampleReuse (envmap.cpp:659-664): std::lower_bound over size + 1 floats
D int envmap_sample_reuse(const float *cdf, int size, float &sample) {
    int lo = 0, n = size + 1;
    while (n > 0) {
        const int half = n >> 1;
        if (cdf[lo + half] < sample) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    int index = lo - 1;
    index = index < 0 ? 0 : index;
    index = index > size - 1 ? size - 1 : index;
    sample = (sample - cdf[index]) / (cdf[index + 1] - cdf[index]);
    return index;
}
D float interval_to_tent(float sample) {  // warp.cpp:143-155
    float sign;
    if (sample < 0.5f) { sign = 1; sample *= 2; }
    else { sign = -1; sample = 2 * (sample - 0.5f); }
    return sign * (1 - __builtin_sqrtf(sample));
}
// internalSampleDirection (envmap.cpp:557-595): direction in the emitter's frame.  DEVIATION: a chosen interval of width 0 — a
// sample component of exactly 0 in front of a black first row or column — is a failed sample (value = 0, pdf = 0) instead of the
// reference's 0 / 0, which its film drops (imageblock.h:150-153) and k_film would keep.
D void envmap_sample_direction(const DevScene &S, float sx, float sy, F3 &d, F3 &value, float &pdf) {
    d = f3s(0.0f); value = f3s(0.0f); pdf = 0.0f;
    const int row = envmap_sample_reuse(S.em_cdf_rows, S.em_h, sy);
    if (S.em_cdf_rows[row + 1] - S.em_cdf_rows[row] == 0) return;
    const float *cols = S.em_cdf_cols + (size_t)row * (S.em_w + 1);
    const int col = envmap_sample_reuse(cols, S.em_w, sx);
    if (cols[col + 1] - cols[col] == 0) return;
    const float posX = (float)col + interval_to_tent(sx), posY = (float)row + interval_to_tent(sy);
    const int xPos = (int)__builtin_floorf(posX), yPos = (int)__builtin_floorf(posY);
    const float dx1 = posX - xPos, dx2 = 1.0f - dx1, dy1 = posY - yPos, dy2 = 1.0f - dy1;
    const F3 value1 = envmap_texel(S, xPos, yPos) * dx2 * dy2 + envmap_texel(S, xPos + 1, yPos) * dx1 * dy2;
    const F3 value2 = envmap_texel(S, xPos, yPos + 1) * dx2 * dy1 + envmap_texel(S, xPos + 1, yPos + 1) * dx1 * dy1;
    value = (value1 + value2) * S.em_scale;
    pdf = (lum3(value1) * S.em_row_weights[envmap_clamp_row(S, yPos)] + lum3(value2) * S.em_row_weights[envmap_clamp_row(S, yPos + 1)]) * S.em_norm;
    float sinPhi, cosPhi, sinTheta, cosTheta;
    dm_sincos(S.em_px * (posX + 0.5f), &sinPhi, &cosPhi);
    dm_sincos(S.em_py * (posY + 0.5f), &sinTheta, &cosTheta);
    d = f3(sinPhi * sinTheta, cosTheta, -cosPhi * sinTheta);
    pdf /= ppg_max(ppg_abs(sinTheta), PPG_EPSILON);
}
// internalPdfDirection (envmap.cpp:598-633): direction in the emitter's frame
D float envmap_pdf_direction(const DevScene &S, F3 d) {
    const float uvx = dm_atan2(d.x, -d.z) * (PPG_INV_PI_F * 0.5f), uvy = dm_acos(d.y) * PPG_INV_PI_F;
    if (!finitef(uvx) || !finitef(uvy)) return 0.0f;
    const float u = uvx * S.em_w - 0.5f, v = uvy * S.em_h - 0.5f;
    const int xPos = (int)__builtin_floorf(u), yPos = (int)__builtin_floorf(v);
    const float dx1 = u - xPos, dx2 = 1.0f - dx1, dy1 = v - yPos, dy2 = 1.0f - dy1;
    const F3 value1 = envmap_texel(S, xPos, yPos) * dx2 * dy2 + envmap_texel(S, xPos + 1, yPos) * dx1 * dy2;
    const F3 value2 = envmap_texel(S, xPos, yPos + 1) * dx2 * dy1 + envmap_texel(S, xPos + 1, yPos + 1) * dx1 * dy1;
    const float sinTheta = __builtin_sqrtf(ppg_max(0.0f, 1 - d.y * d.y));
    return (lum3(value1) * S.em_row_weights[envmap_clamp_row(S, yPos)] + lum3(value2) * S.em_row_weights[envmap_clamp_row(S, yPos + 1)]) * S.em_norm /
           ppg_max(ppg_abs(sinTheta), PPG_EPSILON);
}
// ConstantBackgroundEmitter::sampleDirect (constant.cpp:176-214)
D F3 env_sample_direct(const DevScene &S, F3 ref, F3 refN, float sx, float sy, DirectSample &ds) {
    if (S.env.w == 2.0f) {  // EnvironmentMap::sampleDirect, envmap.cpp:510-538
        F3 dl, value;
        float pdfM;
        envmap_sample_direction(S, sx, sy, dl, value, pdfM);
        const F3 dw = envmap_to_world(S, dl);
        float nearT, farT;
        ds.pdf = 0.0f;
        if (iszero3(value) || pdfM == 0 || !bsphere_intersect(S, ref, dw, nearT, farT) || nearT >= 0 || farT <= 0) return f3s(0.0f);
        ds.pdf = pdfM;
        const F3 p = ref + dw * farT;
        ds.n = norm3(f3(S.bsphere.x, S.bsphere.y, S.bsphere.z) - p);
        ds.dist = farT;
        ds.d = dw;
        const F3 pd = p - ref;
        ds.sdist = len3(pd);
        ds.sd = div3(pd, ds.sdist);
        return div3(value, pdfM);
    }
    F3 d;
    float pdf;
    const bool hasRefN = !(refN.x == 0 && refN.y == 0 && refN.z == 0);
    if (hasRefN) {
        const F3 l = cosine_hemisphere(sx, sy);
        pdf = PPG_INV_PI_F * l.z;
        F3 sF, tF;  // Frame(dRec.refN): coordinateSystem, util.cpp:592-601
        if (ppg_abs(refN.x) > ppg_abs(refN.y)) {
            float invLen = 1.0f / __builtin_sqrtf(refN.x * refN.x + refN.z * refN.z);
            tF = f3(refN.z * invLen, 0.0f, -refN.x * invLen);
        } else {
            float invLen = 1.0f / __builtin_sqrtf(refN.y * refN.y + refN.z * refN.z);
            tF = f3(0.0f, refN.z * invLen, -refN.y * invLen);
        }
        sF = cross3(tF, refN);
        d = sF * l.x + tF * l.y + refN * l.z;
    } else {
        float z = 1.0f - 2.0f * sy;  // warp::squareToUniformSphere, warp.cpp:25-31
        float r = __builtin_sqrtf(ppg_max(0.0f, 1.0f - z * z));
        float sinPhi, cosPhi;
        dm_sincos(2.0f * PPG_PI_F * sx, &sinPhi, &cosPhi);
        d = f3(r * cosPhi, r * sinPhi, z);
        pdf = PPG_INV_PI_F * 0.25f;
    }
    float nearT, farT;
    ds.pdf = 0.0f;
    if (!bsphere_intersect(S, ref, d, nearT, farT)) return f3s(0.0f);
    if (!(nearT < 0 && farT > 0)) return f3s(0.0f);
    const F3 p = ref + d * farT;
    ds.n = norm3(f3(S.bsphere.x, S.bsphere.y, S.bsphere.z) - p);
    ds.d = d;
    ds.dist = farT;
    ds.pdf = pdf;
    const F3 pd = p - ref;
    ds.sdist = len3(pd);
    ds.sd = div3(pd, ds.sdist);
    if (hasRefN && dot3(ds.d, refN) <= 0) return f3s(0.0f);
    return div3(f3(S.env.x, S.env.y, S.env.z), pdf);
}
// Sphere::sampleDirect (sphere.cpp:291-355) and pdfDirect (:357-378), solid-angle measure
D void sphere_sample_direct(const float4 *Q, F3 ref, float sx, float sy, DirectSample &ds) {
    const float4 c4 = Q[0];
    const F3 c = f3(c4.x, c4.y, c4.z);
    const float radius = c4.w;
    const float invSurfaceArea = 1 / (4 * PPG_PI_F * radius * radius);
    const F3 refToCenter = c - ref;
    const float refDist2 = dot3(refToCenter, refToCenter);
    const float invRefDist = 1.0f / __builtin_sqrtf(refDist2);
    const float sinAlpha = radius * invRefDist;
    if (sinAlpha < 1 - PPG_EPSILON) {  // outside: the cone subtended by the sphere
        const float cosAlpha = __builtin_sqrtf(ppg_max(0.0f, 1.0f - sinAlpha * sinAlpha));
        const float cosTheta = (1 - sx) + sx * cosAlpha;  // warp::squareToUniformCone, warp.cpp:54-63
        const float sinTheta = __builtin_sqrtf(ppg_max(0.0f, 1.0f - cosTheta * cosTheta));
        float sinPhi, cosPhi;
        dm_sincos(2.0f * PPG_PI_F * sy, &sinPhi, &cosPhi);
        const F3 lv = f3(cosPhi * sinTheta, sinPhi * sinTheta, cosTheta);
        const F3 a = refToCenter * invRefDist;  // Frame(a): coordinateSystem, util.cpp:592-601
        F3 sF, tF;
        if (ppg_abs(a.x) > ppg_abs(a.y)) {
            const float invLen = 1.0f / __builtin_sqrtf(a.x * a.x + a.z * a.z);
            tF = f3(a.z * invLen, 0.0f, -a.x * invLen);
        } else {
            const float invLen = 1.0f / __builtin_sqrtf(a.y * a.y + a.z * a.z);
            tF = f3(0.0f, a.z * invLen, -a.y * invLen);
        }
        sF = cross3(tF, a);
        ds.d = sF * lv.x + tF * lv.y + a * lv.z;
        ds.pdf = (PPG_INV_PI_F * 0.5f) / (1 - cosAlpha);  // squareToUniformConePdf, warp.h:74-76
        const float projDist = dot3(refToCenter, ds.d);
        const float baseT = refDist2 / projDist;
        const F3 query = ref + ds.d * baseT;
        const F3 queryToCenter = c - query;
        const float queryDist2 = dot3(queryToCenter, queryToCenter);
        const float queryProjDist = dot3(queryToCenter, ds.d);
        const float B = -2 * queryProjDist, Cq = queryDist2 - radius * radius;  // solveQuadratic(1, B, C), util.cpp:447-485
        float nearT;
        const float discrim = B * B - 4.0f * 1.0f * Cq;
        if (discrim < 0) nearT = queryProjDist;
        else {
            const float sqrtDiscrim = __builtin_sqrtf(discrim);
            float temp;
            if (B < 0) temp = -0.5f * (B - sqrtDiscrim);
            else temp = -0.5f * (B + sqrtDiscrim);
            const float x0 = temp / 1.0f, x1 = Cq / temp;
            nearT = x0 > x1 ? x1 : x0;
        }
        ds.dist = baseT + nearT;
        ds.n = norm3(ds.d * nearT - queryToCenter);
        const F3 pd = (c + ds.n * radius) - ref;  // the shadow ray goes to dRec.p (scene.cpp:889-893), not along dRec.d
        ds.sdist = len3(pd);
        ds.sd = div3(pd, ds.sdist);
    } else {  // inside: uniform over the sphere (warp::squareToUniformSphere, warp.cpp:25-31)
        const float z = 1.0f - 2.0f * sy;
        const float r = __builtin_sqrtf(ppg_max(0.0f, 1.0f - z * z));
        float sinPhi, cosPhi;
        dm_sincos(2.0f * PPG_PI_F * sx, &sinPhi, &cosPhi);
        const F3 dv = f3(r * cosPhi, r * sinPhi, z);
        const F3 p = c + dv * radius;
        ds.n = dv;
        F3 dd = p - ref;
        const float dist2 = dot3(dd, dd);
        ds.dist = __builtin_sqrtf(dist2);
        ds.d = div3(dd, ds.dist);
        ds.pdf = invSurfaceArea * dist2 / ppg_abs(dot3(ds.d, ds.n));
        ds.sd = ds.d; ds.sdist = ds.dist;
    }
    if (__float_as_int(Q[3].w)) ds.n = ds.n * -1.0f;
}
D float sphere_pdf_direct(const float4 *Q, F3 ref, F3 d, F3 n, float dist) {
    const float4 c4 = Q[0];
    const F3 refToCenter = f3(c4.x, c4.y, c4.z) - ref;
    const float invRefDist = 1.0f / len3(refToCenter);
    const float sinAlpha = c4.w * invRefDist;
    if (sinAlpha < 1 - PPG_EPSILON) {
        const float cosAlpha = __builtin_sqrtf(ppg_max(0.0f, 1 - sinAlpha * sinAlpha));
        return (PPG_INV_PI_F * 0.5f) / (1 - cosAlpha);
    }
    const float invSurfaceArea = 1 / (4 * PPG_PI_F * c4.w * c4.w);
    return invSurfaceArea * dist * dist / ppg_abs(dot3(d, n));
}
D void disk_concentric(float sx, float sy, float &px, float &py);  // defined below
// Disk::samplePosition (disk.cpp:247-255) / Cylinder::samplePosition (cylinder.cpp:232-246), then Shape::sampleDirect (shape.cpp:97-115):
// the area density (ds.pdf on entry) to solid angle
D void shape_sample_direct(const float4 *Q, F3 ref, float sx, float sy, DirectSample &ds) {
    const float4 q6 = Q[6];
    F3 p, n;
    if (__float_as_int(q6.w) == PPG_SHAPE_DISK) {
        float px, py;
        disk_concentric(sx, sy, px, py);
        p = aff_point(Q, f3(px, py, 0.0f));
        n = f3(0.0f, 0.0f, 1.0f);
    } else {
        float sinTheta, cosTheta;
        dm_sincos(sy * (2 * PPG_PI_F), &sinTheta, &cosTheta);
        p = aff_point(Q, f3(cosTheta * q6.x, sinTheta * q6.x, sx * q6.y));
        n = f3(cosTheta, sinTheta, 0.0f);
    }
    n = norm3(aff_normal(Q + 3, n));
    if (__float_as_int(Q[7].z)) n = n * -1.0f;
    ds.n = n;
    const F3 d = p - ref;
    const float distSquared = dot3(d, d);
    ds.dist = __builtin_sqrtf(distSquared);
    ds.d = div3(d, ds.dist);
    ds.sd = ds.d; ds.sdist = ds.dist;
    const float dp = ppg_abs(dot3(ds.d, ds.n));
    ds.pdf *= dp != 0 ? (distSquared / dp) : 0.0f;
}
// PointEmitter / SpotEmitter / DirectionalEmitter::sampleDirect (point.cpp:131-147, spot.cpp:105-125, 184-200, directional.cpp:159-180)
D F3 delta_sample_direct(const DevScene &S, const float4 *Q, F3 ref, DirectSample &ds) {
    const float4 q0 = Q[0], q1 = Q[1];
    const int type = __float_as_int(q0.w);
    const F3 I = f3(q0.x, q0.y, q0.z);
    ds.is_delta = true;
    if (type == PPG_EMITTER_DIRECTIONAL) {
        const F3 d = f3(q1.x, q1.y, q1.z);
        const F3 diskCenter = f3(S.dir_sphere.x, S.dir_sphere.y, S.dir_sphere.z) - d * S.dir_sphere.w;
        const float distance = dot3(ref - diskCenter, d);
        if (distance < 0) return f3s(0.0f);
        const F3 p = ref - d * distance;
        ds.d = d * -1.0f; ds.n = d; ds.dist = distance; ds.pdf = 1.0f;
        const F3 pd = p - ref;  // the shadow ray goes to dRec.p (scene.cpp:621-623, 889-893)
        ds.sdist = len3(pd);
        ds.sd = div3(pd, ds.sdist);
        return I;
    }
    F3 d = f3(q1.x, q1.y, q1.z) - ref;
    ds.dist = len3(d);
    const float invDist = 1.0f / ds.dist;
    ds.sd = div3(d, ds.dist); ds.sdist = ds.dist;
    d = d * invDist;
    ds.d = d; ds.pdf = 1.0f;
    if (type == PPG_EMITTER_POINT) return I * (invDist * invDist);
    // falloffCurve(trafo.inverse()(-d)): Frame::cosTheta = the z component
    const float4 q2 = Q[2], q3 = Q[3];
    const F3 md = d * -1.0f;
    const float cosTheta = q2.x * md.x + q2.y * md.y + q2.z * md.z;
    if (cosTheta <= q3.x) return f3s(0.0f);
    if (cosTheta >= q3.y) return I * (invDist * invDist);
    return mul3(I, f3s((q1.w - dm_acos(cosTheta)) * q2.w)) * (invDist * invDist);
}
template <bool FULL>
D F3 emitter_sample_direct(const DevScene &S, F3 ref, F3 refN, float sx, float sy, DirectSample &ds) {
    ds.pdf = 0; ds.em_pdf = 0; ds.dist = 0; ds.n = f3s(0.0f); ds.d = f3s(0.0f); ds.is_env = false; ds.is_delta = false; ds.sd = f3s(0.0f); ds.sdist = 0;
    const int n_delta = FULL ? S.n_delta : 0;
    const int n_sel = S.n_emitters + n_delta + (S.env.w != 0 ? 1 : 0);
    if (n_sel == 0) return f3s(0.0f);
    const int e = pmf_sample(S.em_sel_cdf, n_sel + 1, sx);
    const float c0 = S.em_sel_cdf[e], c1 = S.em_sel_cdf[e + 1];
    ds.em_pdf = c1 - c0;
    sx = (sx - c0) / (c1 - c0);  // sampleReuse, pmf.h:183-188
    if (e == S.n_emitters + n_delta) {  // the environment emitter is the last one
        ds.is_env = true;
        return env_sample_direct(S, ref, refN, sx, sy, ds);
    }
    if (FULL && e >= S.n_emitters) return delta_sample_direct(S, S.delta + PPG_DELTA_STRIDE * (e - S.n_emitters), ref, ds);
    const int4 info = S.em_info[e];
    if (info.y == 0) return f3s(0.0f);
    if (info.y < 0) {  // the emitter is an analytic sphere: AreaLight::sampleDirect (area.cpp:158-173) on Sphere::sampleDirect
        sphere_sample_direct(S.spheres + 4 * (-info.y - 1), ref, sx, sy, ds);
        if (!(dot3(ds.d, refN) >= 0 && dot3(ds.d, ds.n) < 0 && ds.pdf != 0)) {
            ds.pdf = 0.0f;
            return f3s(0.0f);
        }
        const float4 r = S.emitters[e];
        return div3(f3(r.x, r.y, r.z), ds.pdf);
    }
    if (PPG_SHAPES && FULL && info.x < 0) {  // a disk or a cylinder (info.y = 1, so that the hit side takes the generic invSurfaceArea density)
        ds.pdf = __int_as_float(info.w);
        shape_sample_direct(S.shapes + PPG_SHAPE_STRIDE * (-info.x - 1), ref, sx, sy, ds);
        if (!(dot3(ds.d, refN) >= 0 && dot3(ds.d, ds.n) < 0 && ds.pdf != 0)) {
            ds.pdf = 0.0f;
            return f3s(0.0f);
        }
        const float4 r = S.emitters[e];
        return div3(f3(r.x, r.y, r.z), ds.pdf);
    }
    const float *acdf = S.em_area_cdf + info.z;
    const int ti = pmf_sample(acdf, info.y + 1, sy);
    const float a0 = acdf[ti], a1 = acdf[ti + 1];
    sy = (sy - a0) / (a1 - a0);
    const float4 *T = S.em_tris + 3 * (size_t)(info.x + ti);
    const F3 p0 = ld3(T), p1 = ld3(T + 1), p2 = ld3(T + 2);
    const float a = __builtin_sqrtf(ppg_max(0.0f, 1.0f - sx));  // warp::squareToUniformTriangle, warp.cpp:76-79
    const float bx = 1 - a, by = a * sy;
    const F3 sideA = p1 - p0, sideB = p2 - p0;
    const F3 p = p0 + sideA * bx + sideB * by;
    if (S.em_normals) {
        const float4 *Nn = S.em_normals + 3 * (size_t)(info.x + ti);
        ds.n = norm3(ld3(Nn) * (1.0f - bx - by) + ld3(Nn + 1) * bx + ld3(Nn + 2) * by);
    } else {
        ds.n = norm3(cross3(sideA, sideB));
    }
    ds.pdf = __int_as_float(info.w);  // invSurfaceArea
    F3 d = p - ref;
    const float distSquared = dot3(d, d);
    ds.dist = __builtin_sqrtf(distSquared);
    ds.d = div3(d, ds.dist);
    ds.sd = ds.d; ds.sdist = ds.dist;
    const float dp = ppg_abs(dot3(ds.d, ds.n));
    ds.pdf *= dp != 0 ? (distSquared / dp) : 0.0f;
    if (!(dot3(ds.d, refN) >= 0 && dot3(ds.d, ds.n) < 0 && ds.pdf != 0)) {
        ds.pdf = 0.0f;
        return f3s(0.0f);
    }
    const float4 r = S.emitters[e];
    return div3(f3(r.x, r.y, r.z), ds.pdf);
}
// Scene::pdfEmitterDirect (scene.cpp:949-952) before the choice probability: the solid-angle density with which emitter em_id (its index in
// the selection table, the environment emitter last) would have been sampled along d from the ray's origin — EnvironmentMap::pdfDirect
// (envmap.cpp:540-552), ConstantBackgroundEmitter::pdfDirect (constant.cpp:216-231), AreaLight::pdfDirect (area.cpp:175-183) on
// Sphere::pdfDirect or Shape::pdfDirect (shape.cpp:117-126).  em_n, em_dist: the emitter's normal and its distance at the hit; refn_ok:
// dot(d, dRec.refN) >= 0.  nee_cos() (dot(d, dRec.refN), -2 without a refN) and ray_origin() (a float4) are called only by the branches
// that need them: the constant environment, and a sphere, whose pdfDirect needs dRec.ref = the previous vertex = the ray's origin.
template <bool FULL, typename NeeCos, typename RayOrigin>
D float emitter_pdf_direct(const DevScene &S, int em_id, F3 d, F3 em_n, float em_dist, bool refn_ok, NeeCos nee_cos, RayOrigin ray_origin) {
    float pdfDirect = 0.0f;
    const float dn = dot3(d, em_n);
    if (FULL && em_id == S.n_emitters + S.n_delta) {
        pdfDirect = S.env.w == 2.0f ? envmap_pdf_direction(S, envmap_to_local(S, d)) : env_pdf_direct(nee_cos());
    } else if (refn_ok && dn < 0) {
        const int4 info = S.em_info[em_id];
        if (FULL && info.y < 0) {
            const float4 ro4 = ray_origin();
            pdfDirect = sphere_pdf_direct(S.spheres + 4 * (-info.y - 1), f3(ro4.x, ro4.y, ro4.z), d, em_n, em_dist);
        } else pdfDirect = __int_as_float(info.w) * (em_dist * em_dist) / ppg_abs(dn);
    }
    return pdfDirect;
}

#if PPG_MEDIA
// ------------------------------------------------------------------------------------------------
// Homogeneous media (medium/homogeneous.cpp) and their phase functions (phase/isotropic.cpp, hg.cpp), restated.  A medium is
// PPG_MEDIUM_STRIDE float4 of DevScene::media.  math::fastexp / fastlog and Spectrum::exp are the deterministic dm_exp / dm_log.
// ------------------------------------------------------------------------------------------------
// exp of a non-positive argument: the deterministic exp clamps its argument at -80, so what lies beyond is flushed to zero here — an
// infinite segment through a medium is opaque, as in the reference; NaN (0 * inf: a channel without extinction over an infinite
// segment, homogeneous.cpp:326, 344) stays NaN, as there
D float medium_exp(float x) {
    if (x != x) return x;
    if (x < -80.0f) return 0.0f;
    return dm_exp(x);
}
D const float4 *medium_record(const float4 *media, unsigned int med) { return media + PPG_MEDIUM_STRIDE * (size_t)(med - 1u); }  // med = 1 + index
// HomogeneousMedium::evalTransmittance (homogeneous.cpp:266-273) over a segment of the given length (ray.maxt - ray.mint)
D F3 medium_transmittance(const float4 *Q, float length) {
    const float4 q1 = Q[1];
    const float negLength = -length;
    return f3(q1.x != 0 ? medium_exp(q1.x * negLength) : 1.0f, q1.y != 0 ? medium_exp(q1.y * negLength) : 1.0f, q1.z != 0 ? medium_exp(q1.z * negLength) : 1.0f);
}
struct MediumSample {
    float t, pdfSuccess, pdfFailure;
    F3 transmittance, sigmaS;
};
// HomogeneousMedium::sampleDistance (homogeneous.cpp:275-352) on the ray (o, d) with mint = 0 and maxt = distSurf; next() is the sampler's
// next1D().  ms.t is sampledDistance as the function leaves it (the distance to the surface on failure).
template <typename Next>
D bool medium_sample_distance(const float4 *Q, F3 o, F3 d, float distSurf, Next next, MediumSample &ms) {
    const float4 q0 = Q[0], q1 = Q[1];
    const int strategy = __float_as_int(Q[2].y);
    const F3 sigmaT = f3(q1.x, q1.y, q1.z);
    const float weight = q0.w;
    float rand = next(), sampledDistance, samplingDensity = q1.w;
    if (rand < weight) {
        rand /= weight;
        if (strategy == PPG_MEDIUM_BALANCE) {
            const int channel = min((int)(next() * 3), 2);
            samplingDensity = comp3(sigmaT, channel);
        }
        sampledDistance = -dm_log(1 - rand) / samplingDensity;
    } else {
        sampledDistance = __builtin_inff();
    }
    bool success = true;
    if (sampledDistance < distSurf) {
        const F3 p = o + d * sampledDistance;
        if (p.x == o.x && p.y == o.y && p.z == o.z) success = false;  // no forward progress
    } else {
        sampledDistance = distSurf;
        success = false;
    }
    float pdfFailure, pdfSuccess;
    if (strategy == PPG_MEDIUM_BALANCE) {
        pdfFailure = 0; pdfSuccess = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float tmp = medium_exp(-comp3(sigmaT, i) * sampledDistance);
            pdfFailure += tmp;
            pdfSuccess += comp3(sigmaT, i) * tmp;
        }
        pdfFailure /= 3;
        pdfSuccess /= 3;
    } else {
        pdfFailure = medium_exp(-samplingDensity * sampledDistance);
        pdfSuccess = samplingDensity * pdfFailure;
    }
    F3 tr = f3(medium_exp(sigmaT.x * -sampledDistance), medium_exp(sigmaT.y * -sampledDistance), medium_exp(sigmaT.z * -sampledDistance));
    ms.pdfSuccess = pdfSuccess * weight;
    ms.pdfFailure = weight * pdfFailure + (1 - weight);
    if (max3(tr) < 1e-20f) tr = f3s(0.0f);
    ms.transmittance = tr;
    ms.sigmaS = f3(q0.x, q0.y, q0.z);
    ms.t = sampledDistance;
    return success;
}
// PhaseFunction::eval: isotropic (warp::squareToUniformSpherePdf) or Henyey-Greenstein (hg.cpp:107-110); wi points back along the ray
D float phase_eval(const float4 *Q, F3 wi, F3 wo) {
    const float4 q2 = Q[2];
    const float INV_FOURPI = 0.07957747154594766788f;
    if (__float_as_int(q2.z) == PPG_PHASE_ISOTROPIC) return INV_FOURPI;
    const float g = q2.x;
    const float temp = 1.0f + g * g + 2.0f * g * dot3(wi, wo);
    return INV_FOURPI * (1 - g * g) / (temp * __builtin_sqrtf(temp));
}
// PhaseFunction::sample(pRec, pdf, sampler) with the 2-D sample (sx, sy): the value is 1, the density is returned (isotropic.cpp:69-74,
// warp.cpp:25-31; hg.cpp:74-105 with Frame(-wi), util.cpp:592-601)
D float phase_sample(const float4 *Q, F3 wi, float sx, float sy, F3 &wo) {
    const float4 q2 = Q[2];
    if (__float_as_int(q2.z) == PPG_PHASE_ISOTROPIC) {
        const float z = 1.0f - 2.0f * sy;
        const float r = __builtin_sqrtf(ppg_max(0.0f, 1.0f - z * z));
        float sinPhi, cosPhi;
        dm_sincos(2.0f * PPG_PI_F * sx, &sinPhi, &cosPhi);
        wo = f3(r * cosPhi, r * sinPhi, z);
        return 0.07957747154594766788f;
    }
    const float g = q2.x;
    float cosTheta;
    if (ppg_abs(g) < PPG_EPSILON) {
        cosTheta = 1 - 2 * sx;
    } else {
        const float sqrTerm = (1 - g * g) / (1 - g + 2 * g * sx);
        cosTheta = (1 + g * g - sqrTerm * sqrTerm) / (2 * g);
    }
    const float sinTheta = __builtin_sqrtf(ppg_max(0.0f, 1.0f - cosTheta * cosTheta));
    float sinPhi, cosPhi;
    dm_sincos(2 * PPG_PI_F * sy, &sinPhi, &cosPhi);
    const F3 a = -wi;
    F3 b, c;
    if (ppg_abs(a.x) > ppg_abs(a.y)) {
        const float invLen = 1.0f / __builtin_sqrtf(a.x * a.x + a.z * a.z);
        c = f3(a.z * invLen, 0.0f, -a.x * invLen);
    } else {
        const float invLen = 1.0f / __builtin_sqrtf(a.y * a.y + a.z * a.z);
        c = f3(0.0f, a.z * invLen, -a.y * invLen);
    }
    b = cross3(c, a);
    wo = b * (sinTheta * cosPhi) + c * (sinTheta * sinPhi) + a * cosTheta;
    return phase_eval(Q, wi, wo);
}
// Intersection::isMediumTransition / getTargetMedium (shape.h): the medium (1 + index, 0 = none) a path continues in when it leaves
// primitive `prim` along d — the exterior one when dot(d, geometric normal) > 0, else the interior one; `word` = 0: no transition
D unsigned int medium_target(unsigned int word, F3 d, F3 geoN) { return dot3(d, geoN) > 0 ? (word >> 16) : (word & 0xffffu); }
D unsigned int medium_word(const DevSceneMedia &S, int prim) { return S.prim_media ? S.prim_media[prim] : 0u; }
#endif

#if PPG_HETMEDIA
// ------------------------------------------------------------------------------------------------
// Heterogeneous media (medium/heterogeneous.cpp, method = woodcock) over const and grid volumes (volume/constvolume.cpp, gridvolume.cpp),
// restated.  A volume is PPG_VOLUME_STRIDE float4 of DevSceneHet::volumes, a medium's heterogeneous record PPG_HET_STRIDE float4 of ::het.
// ------------------------------------------------------------------------------------------------
D const float4 *het_record(const float4 *het, unsigned int med) { return het + PPG_HET_STRIDE * (size_t)(med - 1u); }  // med = 1 + index
D bool het_is(const float4 *Hr) { return __float_as_int(Hr[0].x) != 0; }
// a lookup's cell: m_worldToGrid.transformAffine(p), floorToInt, the bounds test (gridvolume.cpp:338-346); false: the lookup answers 0
struct VolumeCell {
    int i000, sx, sy, sz;  // index of the node (x1, y1, z1) and the strides to x2, y2, z2, in nodes
    float fx, fy, fz;
};
D bool volume_cell(const float4 *V, F3 p_, VolumeCell &c) {
    const float4 q0 = V[0], r0 = V[1], r1 = V[2], r2 = V[3];
    const int rx = __float_as_int(q0.y), ry = __float_as_int(q0.z), rz = __float_as_int(q0.w);
    const float px = r0.x * p_.x + r0.y * p_.y + r0.z * p_.z + r0.w;
    const float py = r1.x * p_.x + r1.y * p_.y + r1.z * p_.z + r1.w;
    const float pz = r2.x * p_.x + r2.y * p_.y + r2.z * p_.z + r2.w;
    // (a NaN coordinate fails this test, where the reference's floorToInt is undefined; anything beyond int's range lies outside as well)
    if (!(px >= 0.0f && py >= 0.0f && pz >= 0.0f && px < (float)rx && py < (float)ry && pz < (float)rz)) return false;
    const int x1 = (int)__builtin_floorf(px), y1 = (int)__builtin_floorf(py), z1 = (int)__builtin_floorf(pz);
    if (x1 + 1 >= rx || y1 + 1 >= ry || z1 + 1 >= rz) return false;
    c.fx = px - x1; c.fy = py - y1; c.fz = pz - z1;
    c.i000 = (z1 * ry + y1) * rx + x1;
    c.sx = 1; c.sy = rx; c.sz = ry * rx;
    return true;
}
// VolumeDataSource::lookupFloat: constvolume.cpp, or gridvolume.cpp:337-388 (EFloat32) with its order of operations
D float volume_lookup_float(const float4 *volumes, const float *pool, int vol, F3 p) {
    const float4 *V = volumes + PPG_VOLUME_STRIDE * (size_t)vol;
    const float4 q4 = V[4];
    if ((__float_as_int(V[0].x) & 0xff) == PPG_VOLUME_CONST) return q4.x;
    VolumeCell c;
    if (!volume_cell(V, p, c)) return 0.0f;
    const float *D0 = pool + (size_t)__float_as_int(q4.w) + c.i000;
    // eight independent loads, issued together
    const float d000 = D0[0], d001 = D0[c.sx], d010 = D0[c.sy], d011 = D0[c.sy + c.sx];
    const float d100 = D0[c.sz], d101 = D0[c.sz + c.sx], d110 = D0[c.sz + c.sy], d111 = D0[c.sz + c.sy + c.sx];
    const float fx = c.fx, fy = c.fy, fz = c.fz, _fx = 1.0f - fx, _fy = 1.0f - fy, _fz = 1.0f - fz;
    return ((d000 * _fx + d001 * fx) * _fy + (d010 * _fx + d011 * fx) * fy) * _fz + ((d100 * _fx + d101 * fx) * _fy + (d110 * _fx + d111 * fx) * fy) * fz;
}
// VolumeDataSource::lookupSpectrum: constvolume.cpp, or gridvolume.cpp's RGB twin of the above (float3 texels)
D F3 volume_lookup_rgb(const float4 *volumes, const float *pool, int vol, F3 p) {
    const float4 *V = volumes + PPG_VOLUME_STRIDE * (size_t)vol;
    const float4 q4 = V[4];
    if ((__float_as_int(V[0].x) & 0xff) == PPG_VOLUME_CONST) return f3(q4.x, q4.y, q4.z);
    VolumeCell c;
    if (!volume_cell(V, p, c)) return f3s(0.0f);
    const float *D0 = pool + (size_t)__float_as_int(q4.w) + 3 * (size_t)c.i000;
    const int sx = 3 * c.sx, sy = 3 * c.sy, sz = 3 * c.sz;
    const float fx = c.fx, fy = c.fy, fz = c.fz, _fx = 1.0f - fx, _fy = 1.0f - fy, _fz = 1.0f - fz;
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d000 = D0[k], d001 = D0[sx + k], d010 = D0[sy + k], d011 = D0[sy + sx + k];
        const float d100 = D0[sz + k], d101 = D0[sz + sx + k], d110 = D0[sz + sy + k], d111 = D0[sz + sy + sx + k];
        r[k] = ((d000 * _fx + d001 * fx) * _fy + (d010 * _fx + d011 * fx) * fy) * _fz + ((d100 * _fx + d101 * fx) * _fy + (d110 * _fx + d111 * fx) * fy) * fz;
    }
    return f3(r[0], r[1], r[2]);
}
// AABB::rayIntersect (aabb.h:317-347), dRcp = 1 / d per component (ray.h).  On the default box (min = +inf, max = -inf) of a const volume
// it answers (-inf, +inf) — and false for a ray with a zero direction component, as the reference does.
D bool aabb_ray_intersect(F3 mn, F3 mx, F3 o, F3 d, float &nearT, float &farT) {
    nearT = -__builtin_inff();
    farT = __builtin_inff();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float origin = comp3(o, i), minVal = comp3(mn, i), maxVal = comp3(mx, i), di = comp3(d, i);
        if (di == 0) {
            if (origin < minVal || origin > maxVal) return false;
        } else {
            const float rcp = 1.0f / di;
            float t1 = (minVal - origin) * rcp, t2 = (maxVal - origin) * rcp;
            if (t1 > t2) { const float tmp = t1; t1 = t2; t2 = tmp; }
            nearT = ppg_max(t1, nearT);  // std::max(t1, nearT) = (t1 < nearT) ? nearT : t1
            farT = ppg_min(t2, farT);
            if (!(nearT <= farT)) return false;
        }
    }
    return true;
}
struct HetSample {
    float t, transmittance;
    F3 sigmaS;
};
// HeterogeneousMedium::sampleDistance, Woodcock branch (heterogeneous.cpp:613-662), on the ray (o, d) over [mint, maxt]; next() is the
// sampler's next1D().  pdfSuccess = pdfFailure = 1; on failure mRec.transmittance = 1, which hs.transmittance says as well.  The loop
// leaves when !(t < maxt), so a NaN cannot keep it running, and after PPG_HETMEDIUM_STEP_CAP steps, as opaque (transmittance 0, no event).
template <typename Next>
D bool hetmedium_sample_distance(const float4 *volumes, const float *pool, const float4 *Hr, F3 o, F3 d, float rmint, float rmaxt, Next next, HetSample &hs) {
    const float4 h0 = Hr[0], h1 = Hr[1], h2 = Hr[2];
    const int densityVol = __float_as_int(h0.x) - 1, albedoVol = __float_as_int(h0.y);
    const float scale = h0.z, invMaxDensity = h0.w;
    hs.t = 0.0f; hs.transmittance = 1.0f; hs.sigmaS = f3s(0.0f);
    float mint, maxt;
    if (!aabb_ray_intersect(f3(h1.x, h1.y, h1.z), f3(h2.x, h2.y, h2.z), o, d, mint, maxt)) return false;
    mint = ppg_max(mint, rmint);
    maxt = ppg_min(maxt, rmaxt);
    float t = mint;
    for (int step = 0; step < PPG_HETMEDIUM_STEP_CAP; ++step) {
        t -= dm_log(1 - next()) * invMaxDensity;
        if (!(t < maxt)) return false;
        const F3 p = o + d * t;
        const float densityAtT = volume_lookup_float(volumes, pool, densityVol, p) * scale;
        if (densityAtT * invMaxDensity > next()) {
            hs.t = t;
            const F3 albedo = volume_lookup_rgb(volumes, pool, albedoVol, p);
            hs.sigmaS = albedo * densityAtT;
            float tr = densityAtT != 0.0f ? 1.0f / densityAtT : 0.0f;
            if (!(ppg_abs(tr) < __builtin_inff())) tr = 0.0f;  // !std::isfinite: prevent rare overflow
            hs.transmittance = tr;
            return true;
        }
    }
    hs.transmittance = 0.0f;
    return false;
}
// HeterogeneousMedium::evalTransmittance with a sampler (heterogeneous.cpp:553-585): the mean of two tracked runs — one of 0, 0.5, 1
template <typename Next>
D float hetmedium_transmittance(const float4 *volumes, const float *pool, const float4 *Hr, F3 o, F3 d, float rmint, float rmaxt, Next next) {
    const float4 h0 = Hr[0], h1 = Hr[1], h2 = Hr[2];
    const int densityVol = __float_as_int(h0.x) - 1;
    const float scale = h0.z, invMaxDensity = h0.w;
    float mint, maxt;
    if (!aabb_ray_intersect(f3(h1.x, h1.y, h1.z), f3(h2.x, h2.y, h2.z), o, d, mint, maxt)) return 1.0f;
    mint = ppg_max(mint, rmint);
    maxt = ppg_min(maxt, rmaxt);
    float result = 0;
    for (int i = 0; i < 2; ++i) {
        float t = mint;
        for (int step = 0; step < PPG_HETMEDIUM_STEP_CAP; ++step) {
            t -= dm_log(1 - next()) * invMaxDensity;
            if (!(t < maxt)) { result += 1; break; }
            const F3 p = o + d * t;
            const float density = volume_lookup_float(volumes, pool, densityVol, p) * scale;
            if (density * invMaxDensity > next()) break;
        }
    }
    return result / 2;
}
// Medium::evalTransmittance of medium `med` (1 + index) over [mint, maxt] of the ray (o, d), whichever kind it is
template <typename Next>
D F3 any_medium_transmittance(const DevSceneHet &S, unsigned int med, F3 o, F3 d, float mint, float maxt, Next next) {
    const float4 *Hr = het_record(S.het, med);
    if (het_is(Hr)) return f3s(hetmedium_transmittance(S.volumes, S.pool, Hr, o, d, mint, maxt, next));
    return medium_transmittance(medium_record(S.media, med), maxt - mint);
}
#endif

// Transform::operator()(Point) (transform.h:108-125) and operator()(Vector) (:175-183)
D F3 xf_point(const float *m, F3 p) {
    float x = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
    float y = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
    float z = m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11];
    float w = m[12] * p.x + m[13] * p.y + m[14] * p.z + m[15];
    if (w == 1.0f) return f3(x, y, z);
    return div3(f3(x, y, z), w);
}
D F3 xf_vec(const float *m, F3 v) {
    return f3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z);
}

// warp.cpp:81-102, 43-52
D void disk_concentric(float sx, float sy, float &px, float &py) {
    float r1 = 2.0f * sx - 1.0f;
    float r2 = 2.0f * sy - 1.0f;
    float phi, r;
    if (r1 == 0 && r2 == 0) {
        r = phi = 0;
    } else if (r1 * r1 > r2 * r2) {
        r = r1;
        phi = (PPG_PI_F / 4.0f) * (r2 / r1);
    } else {
        r = r2;
        phi = (PPG_PI_F / 2.0f) - (r1 / r2) * (PPG_PI_F / 4.0f);
    }
    float c, s;
    dm_sincos(phi, &s, &c);
    px = r * c; py = r * s;
}
// The camera ray of one sample: renderBlock's sample position (GP:1620) + PerspectiveCamera::sampleRayDifferential (or ThinLens's:
// cam.lens, a uniform branch; the pinhole's arithmetic is the same as without it).  Dimensions 0 and 1 of the path key are the position
// in the pixel, 2 and 3 the aperture point of a thin lens; `dim` counts what was drawn.  k_generate, k_fields_sample and the hook
// ppg_debug_camera_rays all call this one function.
D void camera_ray(const DevCamera &cam, unsigned int key, unsigned int pixel, F3 &o, F3 &d, float &mint, float &maxt, unsigned int &dim) {
    dim = 0;
    float u1 = ppg_rand(key, dim++);
    float u2 = ppg_rand(key, dim++);
    int px = (int)(pixel % (unsigned int)cam.width), py = (int)(pixel / (unsigned int)cam.width);
    float sx = (float)px + u1, sy = (float)py + u2;  // GP:1620
    F3 nearP = xf_point(cam.s2c, f3(sx * cam.inv_w, sy * cam.inv_h, 0.0f));
    F3 dl;
    if (cam.lens) {
        // ThinLens::sampleRayDifferential (thinlens.cpp:321-356): the aperture sample is dims 2, 3 (GP:1613-1630); every path has
        // its own origin on the aperture disk
        const float u3 = ppg_rand(key, dim++);
        const float u4 = ppg_rand(key, dim++);
        float ax, ay;
        disk_concentric(u3, u4, ax, ay);
        ax = ax * cam.aperture; ay = ay * cam.aperture;
        const float fDist = cam.focus / nearP.z;
        dl = norm3(nearP * fDist - f3(ax, ay, 0.0f));
        const float *m = cam.c2w;  // Transform::transformAffine(apertureP)
        o = f3(m[0] * ax + m[1] * ay + m[2] * 0.0f + m[3], m[4] * ax + m[5] * ay + m[6] * 0.0f + m[7], m[8] * ax + m[9] * ay + m[10] * 0.0f + m[11]);
    } else {
        dl = norm3(nearP);
        o = f3(cam.c2w[3], cam.c2w[7], cam.c2w[11]);
    }
    float invZ = 1.0f / dl.z;
    mint = cam.near_clip * invZ; maxt = cam.far_clip * invZ;
    d = xf_vec(cam.c2w, dl);
}
D F3 cosine_hemisphere(float sx, float sy) {
    float px, py;
    disk_concentric(sx, sy, px, py);
    float z = __builtin_sqrtf(ppg_max(0.0f, 1.0f - px * px - py * py));
    if (z == 0) z = 1e-10f;
    return f3(px, py, z);
}

// SmoothDiffuse (diffuse.cpp:110-150)
D F3 diffuse_eval(F3 refl, F3 wi, F3 wo) {
    if (wi.z <= 0 || wo.z <= 0) return f3s(0.0f);
    return refl * (PPG_INV_PI_F * wo.z);
}
D float diffuse_pdf(F3 wi, F3 wo) {
    if (wi.z <= 0 || wo.z <= 0) return 0.0f;
    return PPG_INV_PI_F * wo.z;
}

// BSDF dispatch over the supported plugins (include/ppg.h PPG_BSDF_*): diffuse.cpp:110-150, twosided.cpp:100-180
// (one diffuse BRDF on both sides), conductor.cpp:220-290 with material "none" (ideal mirror, delta)
D bool bsdf_is_smooth(int type) { return type != PPG_BSDF_MIRROR; }
D F3 bsdf_eval(int type, F3 refl, F3 wi, F3 wo) {
    if (type == PPG_BSDF_DIFFUSE) return diffuse_eval(refl, wi, wo);
    if (type == PPG_BSDF_TWOSIDED_DIFFUSE) {
        if (wi.z > 0) return diffuse_eval(refl, wi, wo);
        wi.z *= -1; wo.z *= -1;
        return diffuse_eval(refl, wi, wo);
    }
    return f3s(0.0f);
}
D float bsdf_pdf(int type, F3 wi, F3 wo) {
    if (type == PPG_BSDF_DIFFUSE) return diffuse_pdf(wi, wo);
    if (type == PPG_BSDF_TWOSIDED_DIFFUSE) {
        if (wi.z > 0) return diffuse_pdf(wi, wo);
        wi.z *= -1; wo.z *= -1;
        return diffuse_pdf(wi, wo);
    }
    return 0.0f;
}
// returns the sampling weight f·cos/pdf; wo, pdf, delta are outputs
D F3 bsdf_sample(int type, F3 refl, F3 wi, float sx, float sy, F3 &wo, float &pdf, bool &delta) {
    delta = false;
    wo = f3s(0.0f);
    if (type == PPG_BSDF_MIRROR) {
        if (wi.z <= 0) { pdf = 0.0f; return f3s(0.0f); }
        wo = f3(-wi.x, -wi.y, wi.z);  // reflect(wi)
        pdf = 1;
        delta = true;
        return refl;
    }
    bool flipped = false;
    if (type == PPG_BSDF_TWOSIDED_DIFFUSE && wi.z < 0) { wi.z *= -1; flipped = true; }
    if (wi.z <= 0) { pdf = 0.0f; return f3s(0.0f); }
    wo = cosine_hemisphere(sx, sy);
    pdf = PPG_INV_PI_F * wo.z;
    if (flipped && !iszero3(refl) && pdf != 0) wo.z *= -1;
    return refl;
}

// ------------------------------------------------------------------------------------------------
// Full material set (kernel variants instantiated with FULL = true; scenes with only diffuse / two-sided diffuse / mirror
// materials keep the lean functions above).  Expression order follows the cited reference code, like the oracle's.
// ------------------------------------------------------------------------------------------------
// PPG_PARAM_TEXTURES = 0: no kernel of this translation unit calls mat_apply_textures, and Mat has no spec_lum (see mat_spec_lum).  Mat then
// has another layout than in the other translation units.  That is sound only because no Mat ever crosses a translation-unit boundary:
// every function that takes one is __forceinline__ or static, and the library is built without relocatable device code.  Whoever adds a
// non-inline device function taking a Mat, or turns -fgpu-rdc on, must give the switch up first.
#ifndef PPG_PARAM_TEXTURES
#define PPG_PARAM_TEXTURES 1
#endif
// upload-time bit of the record's flags word (beside the PPG_MAT_* of include/ppg.h): mat_eval_null reads a bitmap on this material — a
// mask's opacity, a thin dielectric's specularTransmittance
#define PPG_MATF_NULL_TEXTURED 0x10000
struct Mat {
    int type, flags;          // type normalised: TWOSIDED_DIFFUSE → DIFFUSE + PPG_MAT_TWOSIDED
    F3 refl, spec, eta, k, opacity;
    float alpha, fdr_int;
    const float *rt;          // roughplastic: its rough-transmittance slice, rt_n samples
    int rt_n;
#if PPG_PARAM_TEXTURES
    float spec_lum;           // luminance of the record's specular, likewise, for the kernels in which `spec` may have been read from a bitmap
                              // (mat_apply_textures; plastic.cpp:199-200, roughplastic.cpp:275-276) — see mat_spec_lum
#endif
    float refl_lum;           // luminance of the material record's reflectance = of the texture's average when `refl` was read from a bitmap:
                              // what the plug-ins' configure() derives the component sampling weights from (plastic.cpp:191-204)
#if PPG_MFD
    float alpha_v;            // alphaV (alpha is alphaU); = alpha without a general entry
    unsigned int mfd;         // the entry's PPG_MFDF_* bits, 0 without one
#endif
#if PPG_COAT
    const float4 *coat;       // the material's rows of DevScene::coat when it is coated (ppg_set_coatings), nullptr otherwise
#endif
#if PPG_BLEND
    const float *blend;       // the material's 16 words of DevScene::blend when it is blended (ppg_set_blends), nullptr otherwise
    float bu, bv;             // ... and the hit's its.uv, at which the children's bitmaps and the weight's are looked up
#endif
};
D Mat load_material(const DevScene &S, int id) {
    const float4 *m = S.materials + PPG_MAT_STRIDE * (size_t)id;
    const float4 a = m[0], b = m[1], c = m[2], d = m[3];
    const float4 e = m[4];
    Mat M;
    M.type = (int)a.w; M.flags = __float_as_int(c.w);
    if (M.type == PPG_BSDF_TWOSIDED_DIFFUSE) { M.type = PPG_BSDF_DIFFUSE; M.flags |= PPG_MAT_TWOSIDED; }
    M.refl = f3(a.x, a.y, a.z); M.spec = f3(b.x, b.y, b.z); M.eta = f3(c.x, c.y, c.z); M.k = f3(d.x, d.y, d.z);
    M.alpha = b.w; M.fdr_int = d.w;
    M.opacity = f3(e.x, e.y, e.z);
    M.rt_n = S.rtrans_n;
    M.rt = S.rtrans + (size_t)__float_as_int(e.w) * (size_t)(S.rtrans_n + 1);
    M.refl_lum = a.x * 0.212671f + a.y * 0.715160f + a.z * 0.072169f;
#if PPG_PARAM_TEXTURES
    M.spec_lum = b.x * 0.212671f + b.y * 0.715160f + b.z * 0.072169f;
#endif
#if PPG_MFD
    M.alpha_v = M.alpha; M.mfd = 0u;
    if (S.mfd) {
        const float4 g = S.mfd[id];
        if (__float_as_uint(g.y) & PPG_MFDF_GENERAL) { M.alpha_v = g.x; M.mfd = __float_as_uint(g.y); }
    }
#endif
#if PPG_COAT
    M.coat = nullptr;
    if (S.coat) {
        const float4 *c = S.coat + PPG_COAT_STRIDE * (size_t)id;
        if (__float_as_uint(c[0].w) & PPG_COATF_KIND) M.coat = c;
    }
#endif
#if PPG_BLEND
    M.blend = nullptr; M.bu = 0.0f; M.bv = 0.0f;
    if (S.blend) {
        const float *b = reinterpret_cast<const float *>(S.blend + PPG_BLEND_STRIDE * (size_t)id);
        if (__float_as_uint(b[PPG_BLENDW_BITS]) & PPG_BLENDF_KIND) M.blend = b;
    }
#endif
    return M;
}
// One bitmap lookup of those below, as a CALL: inlined, the three slots at the four places that read them added 53 KB to each FULL kernel
// (k_shade<FULL, MSET_ALL> 112 -> 165 KB), far more than the instruction cache holds; as calls they add about a tenth of that.
static __device__ __attribute__((noinline)) float4 tex_eval_slot(const DevTex *textures, unsigned int slot, float u, float v) {
    const F3 c = tex_eval(textures[slot - 1u], u, v);
    return make_float4(c.x, c.y, c.z, 0.0f);
}
// ... at a hit that has no TexInfo (the surfaces a shadow segment or the search for an emitter passes through): its.uv as fill_isect_tex
// computes it — the interpolated texture coordinates, or the barycentrics on a mesh without them — then the lookup.
static __device__ __attribute__((noinline)) float4 tex_eval_hit(const float2 *uvs, const DevTex *textures, unsigned int slot, int prim, float hu, float hv) {
    float u = hu, v = hv;
    if (uvs) {
        const float2 t0 = uvs[3 * (size_t)prim], t1 = uvs[3 * (size_t)prim + 1], t2 = uvs[3 * (size_t)prim + 2];
        if (tri_has_uvs(t0, t1, t2)) tri_uv_at(t0, t1, t2, f3(1 - hu - hv, hu, hv), u, v);
    }
    return tex_eval_slot(textures, slot, u, v);
}
// Bitmaps on the record's specular / alpha / opacity (ppg_set_material_textures), looked up at (u, v) = its.uv: m_specularReflectance /
// m_specularTransmittance->eval(its), m_alpha->eval(its).average() (roughconductor.cpp:259-262, roughdielectric.cpp:283-286, clamped as
// MicrofacetDistribution does, microfacet.h:135), m_opacity->eval(its) (mask.cpp:115).  The record's row is read again here rather than
// carried from fill_isect_tex: nothing more stays live between the two.  spec_lum / refl_lum keep the record's values (the averages).
D void mat_apply_textures(const DevScene &S, int id, float u, float v, Mat &M) {
    const float4 row = S.materials[PPG_MAT_STRIDE * (size_t)id + 5];
    const unsigned int ts = __float_as_uint(row.y), ta = __float_as_uint(row.z), to = __float_as_uint(row.w);
    if ((ts | ta | to) == 0u) return;
    if (ts) { const float4 t = tex_eval_slot(S.textures, ts, u, v); M.spec = f3(t.x, t.y, t.z); }
    if (ta) { const float4 t = tex_eval_slot(S.textures, ta, u, v); M.alpha = ppg_max((t.x + t.y + t.z) / 3.0f, 1e-4f); }
    if (to) { const float4 t = tex_eval_slot(S.textures, to, u, v); M.opacity = f3(t.x, t.y, t.z); }
}
#if PPG_MFD
// ... and m_alphaV->eval(its).average() of a general entry (ppg_microfacet.alpha_v_texture).  Without an entry alphaV follows alphaU.
D void mat_apply_mfd_textures(const DevScene &S, int id, float u, float v, Mat &M) {
    if (!M.mfd) { M.alpha_v = M.alpha; return; }
    const unsigned int tv = __float_as_uint(S.mfd[id].z);
    if (tv) { const float4 t = tex_eval_slot(S.textures, tv, u, v); M.alpha_v = ppg_max((t.x + t.y + t.z) / 3.0f, 1e-4f); }
}
#endif
// What mat_eval_null reads of a surface passed through: a mask's opacity, a thin dielectric's specularTransmittance.  (Materials of
// analytic spheres carry no slot: h is a triangle wherever one is set.)
D void mat_apply_null_textures(const DevScene &S, const Hit &h, int id, Mat &M) {
    if (!(M.flags & PPG_MATF_NULL_TEXTURED)) return;  // (the flags word came with the record: a constant mask or pane reads nothing more)
    const float4 row = S.materials[PPG_MAT_STRIDE * (size_t)id + 5];
    const unsigned int ts = __float_as_uint(row.y), to = __float_as_uint(row.w);
    if (to) { const float4 t = tex_eval_hit(S.uvs, S.textures, to, h.prim, h.u, h.v); M.opacity = f3(t.x, t.y, t.z); }
    if (ts) { const float4 t = tex_eval_hit(S.uvs, S.textures, ts, h.prim, h.u, h.v); M.spec = f3(t.x, t.y, t.z); }
}
D bool mat_is_smooth(const Mat &M) {
#if PPG_BLEND
    if (M.blend) return (__float_as_uint(M.blend[PPG_BLENDW_BITS]) & PPG_BLENDF_SMOOTH) != 0u;  // smooth if any child is
#endif
#if PPG_COAT
    // a roughcoating's own component is glossy, a coating's is a delta: "nested smooth, or roughcoating"
    if (M.coat && (__float_as_uint(M.coat[0].w) & PPG_COATF_KIND) == 2u) return true;
#endif
#if PPG_LOBES
    if (M.type == PPG_BSDF_ROUGHDIFFUSE || M.type == PPG_BSDF_DIFFTRANS || M.type == PPG_BSDF_PHONG) return true;
#endif
    return M.type == PPG_BSDF_DIFFUSE || M.type == PPG_BSDF_ROUGHCONDUCTOR || M.type == PPG_BSDF_PLASTIC || M.type == PPG_BSDF_ROUGHDIELECTRIC ||
           M.type == PPG_BSDF_ROUGHPLASTIC;
}
D bool mat_two_sided(const Mat &M) {
#if PPG_LOBES
    if (M.type == PPG_BSDF_DIFFTRANS) return false;  // (a transmitter: ppg_set_scene refuses the flag on it)
#endif
    return (M.flags & PPG_MAT_TWOSIDED) && M.type != PPG_BSDF_DIELECTRIC && M.type != PPG_BSDF_THINDIELECTRIC && M.type != PPG_BSDF_ROUGHDIELECTRIC;
}
D bool mat_masked(const Mat &M) { return (M.flags & PPG_MAT_MASK) != 0; }
D bool mat_backside_or_transmission(const Mat &M) {
#if PPG_LOBES
    if (M.type == PPG_BSDF_DIFFTRANS) return true;  // (light on the far side of a diffuse transmitter must not be culled)
#endif
    return (M.flags & (PPG_MAT_TWOSIDED | PPG_MAT_MASK)) || M.type == PPG_BSDF_DIELECTRIC || M.type == PPG_BSDF_THINDIELECTRIC ||
           M.type == PPG_BSDF_ROUGHDIELECTRIC;
}
#if PPG_NORMALMAP_NULL
D bool mat_has_null(const Mat &M) { return mat_masked(M) || M.type == PPG_BSDF_THINDIELECTRIC || M.type == PPG_BSDF_NULL; }  // getType() & ENull
#else
D bool mat_has_null(const Mat &M) { return mat_masked(M) || M.type == PPG_BSDF_THINDIELECTRIC; }  // getType() & ENull
#endif

// sAvg of plastic / roughplastic: the luminance of the RECORD's specular.  The translation unit of k_shade<.., MSET_COMMON>, which never
// looks a parameter texture up, is compiled with PPG_PARAM_TEXTURES = 0 (ppg_inst.hip): the record's value is then M.spec itself and the
// kernel is, instruction for instruction, the one built before these textures existed.
D float mat_spec_lum(const Mat &M) {
#if PPG_PARAM_TEXTURES
    return M.spec_lum;
#else
    return M.spec.x * 0.212671f + M.spec.y * 0.715160f + M.spec.z * 0.072169f;
#endif
}
D F3 cdiv3(F3 a, F3 b) { return f3(a.x / b.x, a.y / b.y, a.z / b.z); }
D F3 safe_sqrt3(F3 s) { return f3(__builtin_sqrtf(ppg_max(0.0f, s.x)), __builtin_sqrtf(ppg_max(0.0f, s.y)), __builtin_sqrtf(ppg_max(0.0f, s.z))); }
D float lum3(F3 s) { return s.x * 0.212671f + s.y * 0.715160f + s.z * 0.072169f; }
D float fsignum(float v) { return (ppg_f2u(v) >> 31) ? -1.0f : 1.0f; }  // math::signum: the FP sign, never zero

// util.cpp:651-681
D float fresnel_dielectric_ext(float cosThetaI_, float &cosThetaT_, float eta) {
    if (eta == 1) { cosThetaT_ = -cosThetaI_; return 0.0f; }
    float scale = (cosThetaI_ > 0) ? 1 / eta : eta, cosThetaTSqr = 1 - (1 - cosThetaI_ * cosThetaI_) * (scale * scale);
    if (cosThetaTSqr <= 0.0f) { cosThetaT_ = 0.0f; return 1.0f; }
    float cosThetaI = ppg_abs(cosThetaI_);
    float cosThetaT = __builtin_sqrtf(cosThetaTSqr);
    float Rs = (cosThetaI - eta * cosThetaT) / (cosThetaI + eta * cosThetaT);
    float Rp = (eta * cosThetaI - cosThetaT) / (eta * cosThetaI + cosThetaT);
    cosThetaT_ = (cosThetaI_ > 0) ? -cosThetaT : cosThetaT;
    return 0.5f * (Rs * Rs + Rp * Rp);
}
D float fresnel_dielectric_ext(float cosThetaI, float eta) { float t; return fresnel_dielectric_ext(cosThetaI, t, eta); }

// util.cpp:739-761
D F3 fresnel_conductor_exact(float cosThetaI, F3 eta, F3 k) {
    float cosThetaI2 = cosThetaI * cosThetaI, sinThetaI2 = 1 - cosThetaI2, sinThetaI4 = sinThetaI2 * sinThetaI2;
    F3 temp1 = mul3(eta, eta) - mul3(k, k) - f3s(sinThetaI2);
    F3 a2pb2 = safe_sqrt3(mul3(temp1, temp1) + mul3(mul3(mul3(k, k), eta), eta) * 4.0f);
    F3 a = safe_sqrt3((a2pb2 + temp1) * 0.5f);
    F3 term1 = a2pb2 + f3s(cosThetaI2), term2 = a * (2 * cosThetaI);
    F3 Rs2 = cdiv3(term1 - term2, term1 + term2);
    F3 term3 = a2pb2 * cosThetaI2 + f3s(sinThetaI4), term4 = term2 * sinThetaI2;
    F3 Rp2 = cdiv3(mul3(Rs2, term3 - term4), term3 + term4);
    return (Rp2 + Rs2) * 0.5f;
}

// math.cpp:25-72
D float mts_erfinv(float x) {
    float w = -dm_log((1.0f - x) * (1.0f + x));
    float p;
    if (w < 5.0f) {
        w = w - 2.5f;
        p = 2.81022636e-08f;
        p = 3.43273939e-07f + p * w;
        p = -3.5233877e-06f + p * w;
        p = -4.39150654e-06f + p * w;
        p = 0.00021858087f + p * w;
        p = -0.00125372503f + p * w;
        p = -0.00417768164f + p * w;
        p = 0.246640727f + p * w;
        p = 1.50140941f + p * w;
    } else {
        w = __builtin_sqrtf(w) - 3.0f;
        p = -0.000200214257f;
        p = 0.000100950558f + p * w;
        p = 0.00134934322f + p * w;
        p = -0.00367342844f + p * w;
        p = 0.00573950773f + p * w;
        p = -0.0076224613f + p * w;
        p = 0.00943887047f + p * w;
        p = 1.00167406f + p * w;
        p = 2.83297682f + p * w;
    }
    return p * x;
}
D float mts_erf(float x) {
    const float a1 = 0.254829592f, a2 = -0.284496736f, a3 = 1.421413741f, a4 = -1.453152027f, a5 = 1.061405429f, p = 0.3275911f;
    const float sign = (ppg_f2u(x) >> 31) ? -1.0f : 1.0f;
    x = ppg_abs(x);
    float t = 1.0f / (1.0f + p * x);
    float y = 1.0f - (((((a5 * t + a4) * t) + a3) * t + a2) * t + a1) * t * dm_exp(-x * x);
    return sign * y;
}

#if !PPG_MFD
// MicrofacetDistribution, isotropic GGX or Beckmann, visible-normal sampling (microfacet.h:191-237, 425-540, 565-690)
struct Mfd { float alpha; bool beckmann; };
D float ggx_eval(Mfd d, F3 m) {
    const float alpha = d.alpha;
    if (m.z <= 0) return 0.0f;
    float cosTheta2 = m.z * m.z;
    float beckmannExponent = ((m.x * m.x) / (alpha * alpha) + (m.y * m.y) / (alpha * alpha)) / cosTheta2;
    float result;
    if (d.beckmann) {
        result = dm_exp(-beckmannExponent) / (PPG_PI_F * alpha * alpha * cosTheta2 * cosTheta2);
        if (beckmannExponent > 80.0f) result = 0;  // (fastexp underflows where dm_exp is clamped: see the extended kernels' copy below)
    } else {
        float root = (1.0f + beckmannExponent) * cosTheta2;
        result = 1.0f / (PPG_PI_F * alpha * alpha * root * root);
    }
    if (result * m.z < 1e-20f) result = 0;
    return result;
}
#define PPG_MAT_MFD(M) Mfd{(M).alpha, ((M).flags & PPG_MAT_BECKMANN) != 0}
#else
// The extended kernels (PPG_MFD): the whole of MicrofacetDistribution (microfacet.h:67-93, 178-565, 700-715) — alphaU / alphaV, the Phong /
// Ashikhmin-Shirley type, sampling of all normals.  Every rough material of such a kernel goes through these functions, also one without
// a general entry: with alphaU == alphaV, ggx or beckmann and visible sampling they perform the float operations of the isotropic
// functions above, as the reference's own isotropic branches do (tests/test_microfacet_general_gpu.py holds them to the oracle bit for bit).
// Out of line (MFD_CALL) where a plug-in calls them from several places: the FULL kernels have no registers or cache left for copies.
#define MFD_CALL static __device__ __attribute__((noinline))
enum { MFD_BECKMANN = 0, MFD_GGX = 1, MFD_PHONG = 2 };
struct Mfd { float alphaU, alphaV, exponentU, exponentV; int type; bool sampleAll; };
D void mfd_phong_exponent(Mfd &d) {  // computePhongExponent, microfacet.h:701-704
    d.exponentU = ppg_max(2.0f / (d.alphaU * d.alphaU) - 2.0f, 0.0f);
    d.exponentV = ppg_max(2.0f / (d.alphaV * d.alphaV) - 2.0f, 0.0f);
}
D Mfd mat_mfd(const Mat &M) {  // MicrofacetDistribution(type, alphaU, alphaV, sampleVisible), microfacet.h:86-93
    Mfd d;
    d.type = (M.mfd & PPG_MFDF_PHONG) ? MFD_PHONG : ((M.flags & PPG_MAT_BECKMANN) ? MFD_BECKMANN : MFD_GGX);
    d.alphaU = ppg_max(M.alpha, 1e-4f); d.alphaV = ppg_max(M.alpha_v, 1e-4f);
    d.sampleAll = (M.mfd & PPG_MFDF_SAMPLE_ALL) != 0u;
    d.exponentU = 0.0f; d.exponentV = 0.0f;
    if (d.type == MFD_PHONG) mfd_phong_exponent(d);
    return d;
}
D Mfd mfd_scale_alpha(Mfd d, float value) {  // scaleAlpha, microfacet.h:178-183
    d.alphaU *= value; d.alphaV *= value;
    if (d.type == MFD_PHONG) mfd_phong_exponent(d);
    return d;
}
#define PPG_MAT_MFD(M) mat_mfd(M)
D float mfd_interpolate_phong_exponent(const Mfd &d, F3 v) {  // microfacet.h:554-565
    const float sinTheta2 = 1.0f - v.z * v.z;
    if (d.alphaU == d.alphaV || sinTheta2 <= 2.93873587705571876e-39f) return d.exponentU;
    float invSinTheta2 = 1 / sinTheta2;
    float cosPhi2 = v.x * v.x * invSinTheta2;
    float sinPhi2 = v.y * v.y * invSinTheta2;
    return d.exponentU * cosPhi2 + d.exponentV * sinPhi2;
}
MFD_CALL float ggx_eval(Mfd d, F3 m) {  // eval, microfacet.h:191-234
    if (m.z <= 0) return 0.0f;
    float cosTheta2 = m.z * m.z;
    float beckmannExponent = ((m.x * m.x) / (d.alphaU * d.alphaU) + (m.y * m.y) / (d.alphaV * d.alphaV)) / cosTheta2;
    float result;
    if (d.type == MFD_BECKMANN) {
        result = dm_exp(-beckmannExponent) / (PPG_PI_F * d.alphaU * d.alphaV * cosTheta2 * cosTheta2);
        // math::fastexp (math.h:185-203) underflows towards 0 where dm_exp is clamped to exp(-80) = 1.8e-35 (ppg_detmath.h), and a normal
        // within 1e-3 of the horizon divides that by cos^4: D came out positive, up to 1e-5 and more, where microfacet.h:203 gives 0.
        // Beyond the clamp the reference's own value falls under its cut (microfacet.h:230) for every alphaU * alphaV < 1e24: exp(-e) /
        // (pi aU aV cos^3) >= 1e-20 with e = tan^2 / a^2 > 80 has no solution below that.  So D = 0 there is the reference's answer.
        if (beckmannExponent > 80.0f) result = 0;
    } else if (d.type == MFD_GGX) {
        float root = (1.0f + beckmannExponent) * cosTheta2;
        result = 1.0f / (PPG_PI_F * d.alphaU * d.alphaV * root * root);
    } else {
        float exponent = mfd_interpolate_phong_exponent(d, m);
        result = __builtin_sqrtf((d.exponentU + 2) * (d.exponentV + 2)) * 0.15915494309189533577f * dm_pow(m.z, exponent);
    }
    if (result * m.z < 1e-20f) result = 0;
    return result;
}
D float mfd_project_roughness(const Mfd &d, F3 v) {  // microfacet.h:541-551
    float invSinTheta2 = 1 / (1.0f - v.z * v.z);
    if (d.alphaU == d.alphaV || invSinTheta2 <= 0) return d.alphaU;
    float cosPhi2 = v.x * v.x * invSinTheta2;
    float sinPhi2 = v.y * v.y * invSinTheta2;
    return __builtin_sqrtf(cosPhi2 * d.alphaU * d.alphaU + sinPhi2 * d.alphaV * d.alphaV);
}
#endif
D float hypot2f(float a, float b) {  // math.cpp:74-86
    float r;
    if (ppg_abs(a) > ppg_abs(b)) { r = b / a; r = ppg_abs(a) * __builtin_sqrtf(1.0f + r * r); }
    else if (b != 0.0f) { r = a / b; r = ppg_abs(b) * __builtin_sqrtf(1.0f + r * r); }
    else r = 0.0f;
    return r;
}
#if !PPG_MFD
D float ggx_smith_g1(Mfd d, F3 v, F3 m) {
    if (dot3(v, m) * v.z <= 0) return 0.0f;
    float temp = 1 - v.z * v.z;
    float tanTheta = temp <= 0.0f ? 0.0f : ppg_abs(__builtin_sqrtf(temp) / v.z);
    if (tanTheta == 0.0f) return 1.0f;
    if (d.beckmann) {
        float a = 1.0f / (d.alpha * tanTheta);
        if (a >= 1.6f) return 1.0f;
        float aSqr = a * a;
        return (3.535f * a + 2.181f * aSqr) / (1.0f + 2.276f * a + 2.577f * aSqr);
    }
    float root = d.alpha * tanTheta;
    return 2.0f / (1.0f + hypot2f(1.0f, root));
}
#else
MFD_CALL float ggx_smith_g1(Mfd d, F3 v, F3 m) {  // smithG1, microfacet.h:477-514
    if (dot3(v, m) * v.z <= 0) return 0.0f;
    float temp = 1 - v.z * v.z;
    float tanTheta = temp <= 0.0f ? 0.0f : ppg_abs(__builtin_sqrtf(temp) / v.z);
    if (tanTheta == 0.0f) return 1.0f;
    float alpha = mfd_project_roughness(d, v);
    if (d.type != MFD_GGX) {  // EPhong, EBeckmann
        float a = 1.0f / (alpha * tanTheta);
        if (a >= 1.6f) return 1.0f;
        float aSqr = a * a;
        return (3.535f * a + 2.181f * aSqr) / (1.0f + 2.276f * a + 2.577f * aSqr);
    }
    float root = alpha * tanTheta;
    return 2.0f / (1.0f + hypot2f(1.0f, root));
}
#endif
D float ggx_pdf_visible(Mfd d, F3 wi, F3 m) {
    if (wi.z == 0) return 0.0f;
    return ggx_smith_g1(d, wi, m) * ppg_abs(dot3(wi, m)) * ggx_eval(d, m) / ppg_abs(wi.z);
}
D void beckmann_sample_visible11(float thetaI, float u, float v, float &sx, float &sy) {  // microfacet.h:565-642
    const float SQRT_PI_INV = 1 / __builtin_sqrtf(PPG_PI_F);
    if (thetaI < 1e-4f) {
        float sinPhi, cosPhi;
        float r = __builtin_sqrtf(-dm_log(1.0f - u));
        dm_sincos(2 * PPG_PI_F * v, &sinPhi, &cosPhi);
        sx = r * cosPhi; sy = r * sinPhi;
        return;
    }
    float tanThetaI = dm_tan(thetaI);
    float cotThetaI = 1 / tanThetaI;
    float a = -1, c = mts_erf(cotThetaI);
    float sample_x = ppg_max(u, 1e-6f);
    float fit = 1 + thetaI * (-0.876f + thetaI * (0.4265f - 0.0594f * thetaI));
    float b = c - (1 + c) * dm_pow(1 - sample_x, fit);
    float normalization = 1 / (1 + c + SQRT_PI_INV * tanThetaI * dm_exp(-cotThetaI * cotThetaI));
    int it = 0;
    while (++it < 10) {
        if (!(b >= a && b <= c)) b = 0.5f * (a + c);
        float invErf = mts_erfinv(b);
        float value = normalization * (1 + b + SQRT_PI_INV * tanThetaI * dm_exp(-invErf * invErf)) - sample_x;
        float derivative = normalization * (1 - invErf * tanThetaI);
        if (ppg_abs(value) < 1e-5f) break;
        if (value > 0) c = b;
        else a = b;
        b -= value / derivative;
    }
    sx = mts_erfinv(b);
    sy = mts_erfinv(2.0f * ppg_max(v, 1e-6f) - 1.0f);
}
D void ggx_sample_visible11(float thetaI, float u, float v, float &sx, float &sy) {
    if (thetaI < 1e-4f) {
        float sinPhi, cosPhi;
        float r = __builtin_sqrtf(ppg_max(0.0f, u / (1 - u)));
        dm_sincos(2 * PPG_PI_F * v, &sinPhi, &cosPhi);
        sx = r * cosPhi; sy = r * sinPhi;
        return;
    }
    float tanThetaI = dm_tan(thetaI);
    float a = 1 / tanThetaI;
    float G1 = 2.0f / (1.0f + __builtin_sqrtf(ppg_max(0.0f, 1.0f + 1.0f / (a * a))));
    float A = 2.0f * u / G1 - 1.0f;
    if (ppg_abs(A) == 1) A -= (A < 0 ? -1.0f : 1.0f) * PPG_EPSILON;
    float tmp = 1.0f / (A * A - 1.0f);
    float B = tanThetaI;
    float Dq = __builtin_sqrtf(ppg_max(0.0f, B * B * tmp * tmp - (A * A - B * B) * tmp));
    float slope_x_1 = B * tmp - Dq;
    float slope_x_2 = B * tmp + Dq;
    sx = (A < 0.0f || slope_x_2 > 1.0f / tanThetaI) ? slope_x_1 : slope_x_2;
    float S;
    if (v > 0.5f) { S = 1.0f; v = 2.0f * (v - 0.5f); }
    else { S = -1.0f; v = 2.0f * (0.5f - v); }
    float z = (v * (v * (v * (-0.365728915865723f) + 0.790235037209296f) - 0.424965825137544f) + 0.000152998850436920f) /
              (v * (v * (v * (v * 0.169507819808272f - 0.397203533833404f) - 0.232500544458471f) + 1.0f) - 0.539825872510702f);
    sy = S * z * __builtin_sqrtf(1.0f + sx * sx);
}
#if !PPG_MFD
D F3 ggx_sample_visible(Mfd d, F3 _wi, float u, float v) {
    const float alpha = d.alpha;
    F3 wi = norm3(f3(alpha * _wi.x, alpha * _wi.y, _wi.z));
    float theta = 0, phi = 0;
    if (wi.z < 0.99999f) {
        theta = dm_acos(wi.z);
        phi = dm_atan2(wi.y, wi.x);
    }
    float sinPhi, cosPhi;
    dm_sincos(phi, &sinPhi, &cosPhi);
    float sx, sy;
    if (d.beckmann) beckmann_sample_visible11(theta, u, v, sx, sy);
    else ggx_sample_visible11(theta, u, v, sx, sy);
    float rx = cosPhi * sx - sinPhi * sy, ry = sinPhi * sx + cosPhi * sy;
    rx *= alpha; ry *= alpha;
    float normalization = 1.0f / __builtin_sqrtf(rx * rx + ry * ry + 1.0f);
    return f3(-rx * normalization, -ry * normalization, normalization);
}
#else
D F3 ggx_sample_visible(Mfd d, F3 _wi, float u, float v) {
    const float alphaU = d.alphaU, alphaV = d.alphaV;  // sampleVisible, microfacet.h:421-459: the two stretches
    F3 wi = norm3(f3(alphaU * _wi.x, alphaV * _wi.y, _wi.z));
    float theta = 0, phi = 0;
    if (wi.z < 0.99999f) {
        theta = dm_acos(wi.z);
        phi = dm_atan2(wi.y, wi.x);
    }
    float sinPhi, cosPhi;
    dm_sincos(phi, &sinPhi, &cosPhi);
    float sx, sy;
    if (d.type == MFD_BECKMANN) beckmann_sample_visible11(theta, u, v, sx, sy);
    else ggx_sample_visible11(theta, u, v, sx, sy);
    float rx = cosPhi * sx - sinPhi * sy, ry = sinPhi * sx + cosPhi * sy;
    rx *= alphaU; ry *= alphaV;
    float normalization = 1.0f / __builtin_sqrtf(rx * rx + ry * ry + 1.0f);
    return f3(-rx * normalization, -ry * normalization, normalization);
}
D void mfd_sample_first_quadrant(const Mfd &d, float u1, float &phi, float &exponent) {  // microfacet.h:707-715
    float cosPhi, sinPhi;
    phi = dm_atan2(__builtin_sqrtf((d.exponentU + 2.0f) / (d.exponentV + 2.0f)) * dm_tan(PPG_PI_F * u1 * 0.5f), 1.0f);  // atan(x) = atan2(x, 1)
    dm_sincos(phi, &sinPhi, &cosPhi);
    exponent = d.exponentU * cosPhi * cosPhi + d.exponentV * sinPhi * sinPhi;
}
// sampleAll, microfacet.h:287-395
D F3 mfd_sample_all(const Mfd &d, float sx, float sy, float &pdf) {
    float cosThetaM = 0.0f;
    float sinPhiM, cosPhiM;
    float alphaSqr;
    if (d.type != MFD_PHONG) {
        if (d.alphaU == d.alphaV) {
            dm_sincos((2.0f * PPG_PI_F) * sy, &sinPhiM, &cosPhiM);
            alphaSqr = d.alphaU * d.alphaU;
        } else {
            float phiM = dm_atan2(d.alphaV / d.alphaU * dm_tan(PPG_PI_F + 2 * PPG_PI_F * sy), 1.0f) + PPG_PI_F * __builtin_floorf(2 * sy + 0.5f);
            dm_sincos(phiM, &sinPhiM, &cosPhiM);
            float cosSc = cosPhiM / d.alphaU, sinSc = sinPhiM / d.alphaV;
            alphaSqr = 1.0f / (cosSc * cosSc + sinSc * sinSc);
        }
        if (d.type == MFD_BECKMANN) {
            float tanThetaMSqr = alphaSqr * -dm_log(1.0f - sx);
            cosThetaM = 1.0f / __builtin_sqrtf(1.0f + tanThetaMSqr);
            pdf = (1.0f - sx) / (PPG_PI_F * d.alphaU * d.alphaV * cosThetaM * cosThetaM * cosThetaM);
        } else {
            float tanThetaMSqr = alphaSqr * sx / (1.0f - sx);
            cosThetaM = 1.0f / __builtin_sqrtf(1.0f + tanThetaMSqr);
            float temp = 1 + tanThetaMSqr / alphaSqr;
            pdf = PPG_INV_PI_F / (d.alphaU * d.alphaV * cosThetaM * cosThetaM * cosThetaM * temp * temp);
        }
    } else {
        float phiM;
        float exponent;
        if (d.alphaU == d.alphaV) {
            phiM = (2.0f * PPG_PI_F) * sy;
            exponent = d.exponentU;
        } else if (sy < 0.25f) {
            mfd_sample_first_quadrant(d, 4 * sy, phiM, exponent);
        } else if (sy < 0.5f) {
            mfd_sample_first_quadrant(d, 4 * (0.5f - sy), phiM, exponent);
            phiM = PPG_PI_F - phiM;
        } else if (sy < 0.75f) {
            mfd_sample_first_quadrant(d, 4 * (sy - 0.5f), phiM, exponent);
            phiM += PPG_PI_F;
        } else {
            mfd_sample_first_quadrant(d, 4 * (1 - sy), phiM, exponent);
            phiM = 2 * PPG_PI_F - phiM;
        }
        dm_sincos(phiM, &sinPhiM, &cosPhiM);
        cosThetaM = dm_pow(sx, 1.0f / (exponent + 2.0f));
        pdf = __builtin_sqrtf((d.exponentU + 2.0f) * (d.exponentV + 2.0f)) * 0.15915494309189533577f * dm_pow(cosThetaM, exponent + 1.0f);
    }
    if (pdf < 1e-20f) pdf = 0;
    float sinThetaM = __builtin_sqrtf(ppg_max(0.0f, 1 - cosThetaM * cosThetaM));
    return f3(sinThetaM * cosPhiM, sinThetaM * sinPhiM, cosThetaM);
}
// sample(wi, sample, pdf) and pdf(wi, m): the m_sampleVisible switch, microfacet.h:240-275.  .w = the density.
MFD_CALL float4 mfd_sample(Mfd d, F3 wi, float sx, float sy) {
    float pdf;
    F3 m;
    if (!d.sampleAll) { m = ggx_sample_visible(d, wi, sx, sy); pdf = ggx_pdf_visible(d, wi, m); }
    else m = mfd_sample_all(d, sx, sy, pdf);
    return make_float4(m.x, m.y, m.z, pdf);
}
D float mfd_pdf(const Mfd &d, F3 wi, F3 m) {
    if (!d.sampleAll) return ggx_pdf_visible(d, wi, m);
    return ggx_eval(d, m) * m.z;  // pdfAll
}
#endif

// plastic.cpp:191-204 (configure) — recomputed per call from the material record, same arithmetic as the oracle's configure()
D float plastic_prob_specular(const Mat &M, float Fi) {
    float dAvg = M.refl_lum, sAvg = mat_spec_lum(M);
    float w = sAvg / (dAvg + sAvg);
    return (Fi * w) / (Fi * w + (1 - Fi) * (1 - w));
}
D F3 plastic_diff_term(const Mat &M) {
    if (M.flags & PPG_MAT_NONLINEAR) return cdiv3(M.refl, f3s(1.0f) - M.refl * M.fdr_int);
    return div3(M.refl, 1 - M.fdr_int);
}

// evalCubicInterp1D (spline.cpp:23-60) on [0, 1], no extrapolation
D float cubic_interp_1d(float x, const float *values, int size) {
    if (!(x >= 0.0f && x <= 1.0f)) return 0.0f;
    float t = ((x - 0.0f) * (float)(size - 1)) / (1.0f - 0.0f);
    int k = (int)t;
    k = k < size - 2 ? k : size - 2;
    k = k > 0 ? k : 0;
    const float f0 = values[k], f1 = values[k + 1];
    float d0, d1;
    if (k > 0) d0 = 0.5f * (values[k + 1] - values[k - 1]);
    else d0 = values[k + 1] - values[k];
    if (k + 2 < size) d1 = 0.5f * (values[k + 2] - values[k]);
    else d1 = values[k + 1] - values[k];
    t = t - (float)k;
    const float t2 = t * t, t3 = t2 * t;
    return (2 * t3 - 3 * t2 + 1) * f0 + (-2 * t3 + 3 * t2) * f1 + (t3 - 2 * t2 + t) * d0 + (t3 - t2) * d1;
}
// roughplastic: m_externalRoughTransmittance->eval(cosTheta, alpha), eta and alpha fixed (rtrans.h:185-196, 233)
D float rough_T(const Mat &M, float cosTheta) {
    const float warped = dm_pow(ppg_abs(cosTheta), 0.25f);
    if (!(cosTheta >= 0)) return 0.0f;
    return ppg_min(1.0f, ppg_max(0.0f, cubic_interp_1d(warped, M.rt, M.rt_n)));
}
D float roughplastic_prob_specular(const Mat &M, float cosThetaI) {  // roughplastic.cpp:406-412
    const float dAvg = M.refl_lum, sAvg = mat_spec_lum(M);
    const float w = sAvg / (dAvg + sAvg);
    const float pS = 1 - rough_T(M, cosThetaI);
    return (pS * w) / (pS * w + (1 - pS) * (1 - w));
}

// thindielectric.cpp:160-164: slab reflectance incl. internal reflections R' = R + TRT + TR^3T + ..
D float thin_R(const Mat &M, float cosThetaI) {
    float Rr = fresnel_dielectric_ext(ppg_abs(cosThetaI), M.eta.x), Tt = 1 - Rr;
    if (Rr < 1) Rr += Tt * Tt * Rr / (1 - Rr * Rr);
    return Rr;
}
// BSDF::eval(BSDFSamplingRecord(its, -wo, wo), EDiscrete) restricted to the null component: what a ray going straight through keeps
D F3 mat_eval_null(const Mat &M, float cosThetaI) {
    if (mat_masked(M)) return f3s(1.0f) - M.opacity;  // mask.cpp:115-116
#if PPG_NORMALMAP_NULL
    if (M.type == PPG_BSDF_NULL) return f3s(1.0f);  // null.cpp:43-45 (ppg_set_scene refuses a mask around it)
#endif
    return M.spec * (1 - thin_R(M, cosThetaI));
}

#if PPG_LOBES
// ------------------------------------------------------------------------------------------------
// The lobes kernels (PPG_LOBES): roughdiffuse (roughdiffuse.cpp:128-252), difftrans (difftrans.cpp:76-116) and phong (phong.cpp:122-240),
// each float operation in the plug-in's order.  Out of line (MFD_CALL), scalars in and out: shade_one<FULL> has no registers left for
// inlined copies.  All three are smooth, never delta, never null, eta = 1, and draw nothing from the path's sampler.
// ------------------------------------------------------------------------------------------------
D float frame_sin_theta(F3 v) {  // Frame::sinTheta, frame.h:107-118
    const float temp = 1.0f - v.z * v.z;
    if (temp <= 0.0f) return 0.0f;
    return __builtin_sqrtf(temp);
}
D float clamp_unit(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }  // math::clamp(v, -1, 1)
// std::pow where exp(y log x) has no answer: pow(x, 0) = 1 — a phong exponent of 0 —, pow(0, y > 0) = 0 — sample.y = 0 —; x >= 0 always
D float lobe_pow(float x, float y) {
    if (y == 0.0f) return 1.0f;
    if (x == 0.0f) return 0.0f;
    return dm_pow(x, y);
}
MFD_CALL F3 roughdiffuse_eval(F3 rho, float alpha, bool fast, F3 wi, F3 wo) {  // roughdiffuse.cpp:128-218
    if (wi.z <= 0 || wo.z <= 0) return f3s(0.0f);
    const float conversionFactor = 1 / __builtin_sqrtf(2.0f);
    const float sigma = alpha * conversionFactor;
    const float sigma2 = sigma * sigma;
    const float sinThetaI = frame_sin_theta(wi), sinThetaO = frame_sin_theta(wo);
    float cosPhiDiff = 0;
    if (sinThetaI > PPG_EPSILON && sinThetaO > PPG_EPSILON) {  // Frame::sinPhi / cosPhi, frame.h:140-154
        const float sinPhiI = clamp_unit(wi.y / sinThetaI), cosPhiI = clamp_unit(wi.x / sinThetaI);
        const float sinPhiO = clamp_unit(wo.y / sinThetaO), cosPhiO = clamp_unit(wo.x / sinThetaO);
        cosPhiDiff = cosPhiI * cosPhiO + sinPhiI * sinPhiO;
    }
    if (fast) {
        const float A = 1.0f - 0.5f * sigma2 / (sigma2 + 0.33f), B = 0.45f * sigma2 / (sigma2 + 0.09f);
        float sinAlpha, tanBeta;
        if (wi.z > wo.z) { sinAlpha = sinThetaO; tanBeta = sinThetaI / wi.z; }
        else { sinAlpha = sinThetaI; tanBeta = sinThetaO / wo.z; }
        return rho * (PPG_INV_PI_F * wo.z * (A + B * ppg_max(cosPhiDiff, 0.0f) * sinAlpha * tanBeta));
    }
    const float thetaI = dm_acos(wi.z), thetaO = dm_acos(wo.z);
    const float alphaA = ppg_max(thetaI, thetaO), beta = ppg_min(thetaI, thetaO);
    float sinAlpha, sinBeta, tanBeta;
    if (wi.z > wo.z) { sinAlpha = sinThetaO; sinBeta = sinThetaI; tanBeta = sinThetaI / wi.z; }
    else { sinAlpha = sinThetaI; sinBeta = sinThetaO; tanBeta = sinThetaO / wo.z; }
    const float tmp = sigma2 / (sigma2 + 0.09f), tmp2 = (4 * PPG_INV_PI_F * PPG_INV_PI_F) * alphaA * beta, tmp3 = 2 * beta * PPG_INV_PI_F;
    const float C1 = 1.0f - 0.5f * sigma2 / (sigma2 + 0.33f);
    float C2 = 0.45f * tmp;
    const float C3 = 0.125f * tmp * tmp2 * tmp2, C4 = 0.17f * sigma2 / (sigma2 + 0.13f);
    if (cosPhiDiff > 0) C2 *= sinAlpha;
    else C2 *= sinAlpha - tmp3 * tmp3 * tmp3;
    const float tanHalf = (sinAlpha + sinBeta) / (__builtin_sqrtf(ppg_max(0.0f, 1.0f - sinAlpha * sinAlpha)) + __builtin_sqrtf(ppg_max(0.0f, 1.0f - sinBeta * sinBeta)));
    const F3 snglScat = rho * (C1 + cosPhiDiff * C2 * tanBeta + (1.0f - ppg_abs(cosPhiDiff)) * C3 * tanHalf);
    const F3 dblScat = mul3(rho, rho) * (C4 * (1.0f - cosPhiDiff * tmp3 * tmp3));
    return (snglScat + dblScat) * (PPG_INV_PI_F * wo.z);
}
// m_specularSamplingWeight (phong.cpp:97-99), from the luminances of the RECORD's values, as plastic_prob_specular takes them
D float phong_weight(const Mat &M) {
    const float dAvg = M.refl_lum, sAvg = mat_spec_lum(M);
    return sAvg / (dAvg + sAvg);
}
MFD_CALL F3 phong_eval(F3 diff, F3 spec, float exponent, F3 wi, F3 wo) {  // phong.cpp:122-147
    if (wi.z <= 0 || wo.z <= 0) return f3s(0.0f);
    F3 result = f3s(0.0f);
    const float alpha = dot3(wo, f3(-wi.x, -wi.y, wi.z));
    if (alpha > 0.0f) result = result + spec * ((exponent + 2) * 0.15915494309189533577f * lobe_pow(alpha, exponent));
    result = result + diff * PPG_INV_PI_F;
    return result * wo.z;
}
MFD_CALL float phong_pdf(float weight, float exponent, F3 wi, F3 wo) {  // phong.cpp:149-181
    if (wi.z <= 0 || wo.z <= 0) return 0.0f;
    const float diffuseProb = PPG_INV_PI_F * wo.z;
    float specProb = 0.0f;
    const float alpha = dot3(wo, f3(-wi.x, -wi.y, wi.z));
    if (alpha > 0) specProb = lobe_pow(alpha, exponent) * (exponent + 1.0f) / (2.0f * PPG_PI_F);
    return weight * specProb + (1 - weight) * diffuseProb;
}
// the direction of phong.cpp:183-231 (.w = 0: the rotated lobe direction lies below the surface)
MFD_CALL float4 phong_sample_dir(float weight, float exponent, F3 wi, float sx, float sy) {
    F3 wo;
    if (sx <= weight) {
        sx /= weight;
        const F3 n = f3(-wi.x, -wi.y, wi.z);
        const float sinAlpha = __builtin_sqrtf(ppg_max(0.0f, 1 - lobe_pow(sy, 2 / (exponent + 1))));
        const float cosAlpha = lobe_pow(sy, 1 / (exponent + 1));
        const float phi = (2.0f * PPG_PI_F) * sx;
        float sinPhi, cosPhi;
        dm_sincos(phi, &sinPhi, &cosPhi);
        const F3 l = f3(sinAlpha * cosPhi, sinAlpha * sinPhi, cosAlpha);
        F3 tF;  // Frame(R): coordinateSystem, util.cpp:592-601
        if (ppg_abs(n.x) > ppg_abs(n.y)) {
            const float invLen = 1.0f / __builtin_sqrtf(n.x * n.x + n.z * n.z);
            tF = f3(n.z * invLen, 0.0f, -n.x * invLen);
        } else {
            const float invLen = 1.0f / __builtin_sqrtf(n.y * n.y + n.z * n.z);
            tF = f3(0.0f, n.z * invLen, -n.y * invLen);
        }
        const F3 sF = cross3(tF, n);
        wo = sF * l.x + tF * l.y + n * l.z;
        if (wo.z <= 0) return make_float4(wo.x, wo.y, wo.z, 0.0f);
    } else {
        sx = (sx - weight) / (1 - weight);
        wo = cosine_hemisphere(sx, sy);
    }
    return make_float4(wo.x, wo.y, wo.z, 1.0f);
}
#endif

// one-sided plugins, solid-angle measure
D F3 mat_eval_one(const Mat &M, F3 wi, F3 wo) {
    if (M.type == PPG_BSDF_DIFFUSE) return diffuse_eval(M.refl, wi, wo);
    if (M.type == PPG_BSDF_ROUGHCONDUCTOR) {  // roughconductor.cpp:247-282
        if (wi.z <= 0 || wo.z <= 0) return f3s(0.0f);
        F3 H = norm3(wo + wi);
        const Mfd distr = PPG_MAT_MFD(M);
        const float Dm = ggx_eval(distr, H);
        if (Dm == 0) return f3s(0.0f);
        const F3 F = mul3(fresnel_conductor_exact(dot3(wi, H), M.eta, M.k), M.refl);
        const float G = ggx_smith_g1(distr, wi, H) * ggx_smith_g1(distr, wo, H);
        float model = Dm * G / (4.0f * wi.z);
        return F * model;
    }
    if (M.type == PPG_BSDF_ROUGHDIELECTRIC) {  // roughdielectric.cpp:268-340
        if (wi.z == 0) return f3s(0.0f);
        const float m_eta = M.eta.x, m_invEta = 1 / m_eta;
        const bool reflect = wi.z * wo.z > 0;
        F3 H;
        if (reflect) H = norm3(wo + wi);
        else {
            float eta = wi.z > 0 ? m_eta : m_invEta;
            H = norm3(wi + wo * eta);
        }
        H = H * fsignum(H.z);
        const Mfd distr = PPG_MAT_MFD(M);
        const float Dm = ggx_eval(distr, H);
        if (Dm == 0) return f3s(0.0f);
        const float F = fresnel_dielectric_ext(dot3(wi, H), m_eta);
        const float G = ggx_smith_g1(distr, wi, H) * ggx_smith_g1(distr, wo, H);
        if (reflect) {
            float value = F * Dm * G / (4.0f * ppg_abs(wi.z));
            return M.refl * value;
        }
        float eta = wi.z > 0.0f ? m_eta : m_invEta;
        float sqrtDenom = dot3(wi, H) + eta * dot3(wo, H);
        float value = ((1 - F) * Dm * G * eta * eta * dot3(wi, H) * dot3(wo, H)) / (wi.z * sqrtDenom * sqrtDenom);
        float factor = wi.z > 0 ? m_invEta : m_eta;
        return M.spec * ppg_abs(value * factor * factor);
    }
    if (M.type == PPG_BSDF_ROUGHPLASTIC) {  // roughplastic.cpp:330-384
        if (wi.z <= 0 || wo.z <= 0) return f3s(0.0f);
        const Mfd distr = PPG_MAT_MFD(M);
        const F3 H = norm3(wo + wi);
        const float Dm = ggx_eval(distr, H);
        const float F = fresnel_dielectric_ext(dot3(wi, H), M.eta.x);
        const float G = ggx_smith_g1(distr, wi, H) * ggx_smith_g1(distr, wo, H);
        const float value = F * Dm * G / (4.0f * wi.z);
        const F3 result = M.spec * value;
        const float T12 = rough_T(M, wi.z), T21 = rough_T(M, wo.z);
        const float invEta2 = 1.0f / (M.eta.x * M.eta.x);
        return result + plastic_diff_term(M) * (PPG_INV_PI_F * wo.z * T12 * T21 * invEta2);
    }
    if (M.type == PPG_BSDF_PLASTIC) {  // plastic.cpp:247-281, diffuse component
        if (wo.z <= 0 || wi.z <= 0) return f3s(0.0f);
        float Fi = fresnel_dielectric_ext(wi.z, M.eta.x);
        float Fo = fresnel_dielectric_ext(wo.z, M.eta.x);
        const float invEta2 = 1 / (M.eta.x * M.eta.x);
        return plastic_diff_term(M) * ((PPG_INV_PI_F * wo.z) * invEta2 * (1 - Fi) * (1 - Fo));
    }
#if PPG_LOBES
    if (M.type == PPG_BSDF_ROUGHDIFFUSE) return roughdiffuse_eval(M.refl, M.alpha, (M.flags & PPG_MAT_FAST_APPROX) != 0, wi, wo);
    if (M.type == PPG_BSDF_DIFFTRANS) {  // difftrans.cpp:76-83
        if (wi.z * wo.z >= 0) return f3s(0.0f);
        return M.refl * (PPG_INV_PI_F * ppg_abs(wo.z));
    }
    if (M.type == PPG_BSDF_PHONG) return phong_eval(M.refl, M.spec, M.alpha, wi, wo);
#endif
    return f3s(0.0f);
}
D float mat_pdf_one(const Mat &M, F3 wi, F3 wo) {
    if (M.type == PPG_BSDF_DIFFUSE) return diffuse_pdf(wi, wo);
    if (M.type == PPG_BSDF_ROUGHCONDUCTOR) {  // roughconductor.cpp:284-307
        if (wi.z <= 0 || wo.z <= 0) return 0.0f;
        F3 H = norm3(wo + wi);
        const Mfd distr = PPG_MAT_MFD(M);
#if PPG_MFD
        if (distr.sampleAll) return mfd_pdf(distr, wi, H) / (4 * ppg_abs(dot3(wo, H)));  // roughconductor.cpp:316-320
#endif
        return ggx_eval(distr, H) * ggx_smith_g1(distr, wi, H) / (4.0f * wi.z);
    }
    if (M.type == PPG_BSDF_ROUGHDIELECTRIC) {  // roughdielectric.cpp:342-418
        const float m_eta = M.eta.x, m_invEta = 1 / m_eta;
        const bool reflect = wi.z * wo.z > 0;
        F3 H;
        float dwh_dwo;
        if (reflect) {
            H = norm3(wo + wi);
            dwh_dwo = 1.0f / (4.0f * dot3(wo, H));
        } else {
            float eta = wi.z > 0 ? m_eta : m_invEta;
            H = norm3(wi + wo * eta);
            float sqrtDenom = dot3(wi, H) + eta * dot3(wo, H);
            dwh_dwo = (eta * eta * dot3(wo, H)) / (sqrtDenom * sqrtDenom);
        }
        H = H * fsignum(H.z);
#if PPG_MFD
        Mfd sampleDistr = mat_mfd(M);  // Walter's trick, roughdielectric.cpp:406-411
        if (sampleDistr.sampleAll) sampleDistr = mfd_scale_alpha(sampleDistr, 1.2f - 0.2f * __builtin_sqrtf(ppg_abs(wi.z)));
        float prob = mfd_pdf(sampleDistr, wi * fsignum(wi.z), H);
#else
        const Mfd distr = PPG_MAT_MFD(M);
        float prob = ggx_pdf_visible(distr, wi * fsignum(wi.z), H);
#endif
        float F = fresnel_dielectric_ext(dot3(wi, H), m_eta);
        prob *= reflect ? F : (1 - F);
        return ppg_abs(prob * dwh_dwo);
    }
    if (M.type == PPG_BSDF_ROUGHPLASTIC) {  // roughplastic.cpp:386-437
        if (wi.z <= 0 || wo.z <= 0) return 0.0f;
        const Mfd distr = PPG_MAT_MFD(M);
        const F3 H = norm3(wo + wi);
        const float pS = roughplastic_prob_specular(M, wi.z), pD = 1 - pS;
        const float dwh_dwo = 1.0f / (4.0f * dot3(wo, H));
#if PPG_MFD
        const float prob = mfd_pdf(distr, wi, H);
#else
        const float prob = ggx_pdf_visible(distr, wi, H);
#endif
        float result = prob * dwh_dwo * pS;
        result += pD * (PPG_INV_PI_F * wo.z);
        return result;
    }
    if (M.type == PPG_BSDF_PLASTIC) {  // plastic.cpp:283-311
        if (wo.z <= 0 || wi.z <= 0) return 0.0f;
        float Fi = fresnel_dielectric_ext(wi.z, M.eta.x);
        return (PPG_INV_PI_F * wo.z) * (1 - plastic_prob_specular(M, Fi));
    }
#if PPG_LOBES
    if (M.type == PPG_BSDF_ROUGHDIFFUSE) return diffuse_pdf(wi, wo);  // roughdiffuse.cpp:220-227
    if (M.type == PPG_BSDF_DIFFTRANS) {  // difftrans.cpp:85-91
        if (wi.z * wo.z >= 0) return 0.0f;
        return ppg_abs(wo.z) * PPG_INV_PI_F;
    }
    if (M.type == PPG_BSDF_PHONG) return phong_pdf(phong_weight(M), M.alpha, wi, wo);
#endif
    return 0.0f;
}
#if PPG_COAT
// The coat kernels (PPG_COAT) reach the nested BSDF's eval() / pdf() through real calls: a coat evaluates them once more on the refracted
// pair, roughcoating's sample() after the nested sample() as well, and the FULL kernels have neither registers nor instruction cache for
// further inlined copies of the material switch.  The arithmetic is that of the inlined functions: uncoated materials keep their bits.
MFD_CALL F3 mat_eval_one_call(Mat M, F3 wi, F3 wo) { return mat_eval_one(M, wi, wo); }
MFD_CALL float mat_pdf_one_call(Mat M, F3 wi, F3 wo) { return mat_pdf_one(M, wi, wo); }
#define MAT_EVAL_ONE mat_eval_one_call
#define MAT_PDF_ONE mat_pdf_one_call
#else
#define MAT_EVAL_ONE mat_eval_one
#define MAT_PDF_ONE mat_pdf_one
#endif
D F3 mat_sample_one(const Mat &M, F3 wi, float sx, float sy, F3 &wo, float &pdf, bool &delta, float &eta, bool &isnull, unsigned int key,
                    unsigned int &dim) {
    delta = false; eta = 1.0f; pdf = 0.0f; wo = f3s(0.0f); isnull = false;
    switch (M.type) {
        case PPG_BSDF_DIFFUSE:
            if (wi.z <= 0) return f3s(0.0f);
            wo = cosine_hemisphere(sx, sy);
            pdf = PPG_INV_PI_F * wo.z;
            return M.refl;
        case PPG_BSDF_MIRROR:
        case PPG_BSDF_CONDUCTOR:  // conductor.cpp:268-284
            if (wi.z <= 0) return f3s(0.0f);
            wo = f3(-wi.x, -wi.y, wi.z);
            delta = true;
            pdf = 1;
            return mul3(M.refl, fresnel_conductor_exact(wi.z, M.eta, M.k));
        case PPG_BSDF_ROUGHCONDUCTOR: {  // roughconductor.cpp:367-415
            if (wi.z < 0) return f3s(0.0f);
            const Mfd distr = PPG_MAT_MFD(M);
#if PPG_MFD
            const float4 ms = mfd_sample(distr, wi, sx, sy);
            F3 m = f3(ms.x, ms.y, ms.z);
            pdf = ms.w;
#else
            F3 m = ggx_sample_visible(distr, wi, sx, sy);
            pdf = ggx_pdf_visible(distr, wi, m);
#endif
            if (pdf == 0) return f3s(0.0f);
            wo = m * (2 * dot3(wi, m)) - wi;
            if (wo.z <= 0) return f3s(0.0f);
            F3 F = mul3(fresnel_conductor_exact(dot3(wi, m), M.eta, M.k), M.refl);
#if PPG_MFD
            float weight;
            if (!distr.sampleAll) weight = ggx_smith_g1(distr, wo, m);
            else weight = ggx_eval(distr, m) * (ggx_smith_g1(distr, wi, m) * ggx_smith_g1(distr, wo, m)) * dot3(wi, m) / (pdf * wi.z);
#else
            float weight = ggx_smith_g1(distr, wo, m);
#endif
            pdf /= 4.0f * dot3(wo, m);
            return F * weight;
        }
        case PPG_BSDF_ROUGHPLASTIC: {  // roughplastic.cpp:439-501
            if (wi.z <= 0) return f3s(0.0f);
            const Mfd distr = PPG_MAT_MFD(M);
            const float pS = roughplastic_prob_specular(M, wi.z);
            if (sy < pS) {
                sy /= pS;
#if PPG_MFD
                const float4 ms = mfd_sample(distr, wi, sx, sy);
                const F3 m = f3(ms.x, ms.y, ms.z);
#else
                const F3 m = ggx_sample_visible(distr, wi, sx, sy);
#endif
                wo = m * (2 * dot3(wi, m)) - wi;
                if (wo.z <= 0) return f3s(0.0f);
            } else {
                sy = (sy - pS) / (1 - pS);
                wo = cosine_hemisphere(sx, sy);
            }
            pdf = MAT_PDF_ONE(M, wi, wo);
            if (pdf == 0) return f3s(0.0f);
            return div3(MAT_EVAL_ONE(M, wi, wo), pdf);
        }
        case PPG_BSDF_PLASTIC: {  // plastic.cpp:368-425
            if (wi.z <= 0) return f3s(0.0f);
            float Fi = fresnel_dielectric_ext(wi.z, M.eta.x);
            float pS = plastic_prob_specular(M, Fi);
            if (sx < pS) {
                delta = true;
                wo = f3(-wi.x, -wi.y, wi.z);
                pdf = pS;
                return div3(M.spec * Fi, pS);
            }
            wo = cosine_hemisphere((sx - pS) / (1 - pS), sy);
            float Fo = fresnel_dielectric_ext(wo.z, M.eta.x);
            pdf = (1 - pS) * (PPG_INV_PI_F * wo.z);
            const float invEta2 = 1 / (M.eta.x * M.eta.x);
            return plastic_diff_term(M) * (invEta2 * (1 - Fi) * (1 - Fo) / (1 - pS));
        }
        case PPG_BSDF_DIELECTRIC: {  // dielectric.cpp:271-312, ERadiance
            float cosThetaT;
            const float e = M.eta.x, invEta = 1 / e;
            float F = fresnel_dielectric_ext(wi.z, cosThetaT, e);
            delta = true;
            if (sx <= F) {
                wo = f3(-wi.x, -wi.y, wi.z);
                pdf = F;
                return M.refl;
            }
            float scale = -(cosThetaT < 0 ? invEta : e);
            wo = f3(scale * wi.x, scale * wi.y, cosThetaT);
            eta = cosThetaT < 0 ? e : invEta;
            pdf = 1 - F;
            float factor = cosThetaT < 0 ? invEta : e;
            return M.spec * (factor * factor);
        }
        case PPG_BSDF_ROUGHDIELECTRIC: {  // roughdielectric.cpp:514-606
            const float m_eta = M.eta.x, m_invEta = 1 / m_eta;
            const Mfd distr = PPG_MAT_MFD(M);
            const F3 wis = wi * fsignum(wi.z);
#if PPG_MFD
            Mfd sampleDistr = distr;  // Walter's trick, roughdielectric.cpp:535-540
            if (distr.sampleAll) sampleDistr = mfd_scale_alpha(distr, 1.2f - 0.2f * __builtin_sqrtf(ppg_abs(wi.z)));
            const float4 ms = mfd_sample(sampleDistr, wis, sx, sy);
            const F3 m = f3(ms.x, ms.y, ms.z);
            const float microfacetPDF = ms.w;
#else
            const F3 m = ggx_sample_visible(distr, wis, sx, sy);
            const float microfacetPDF = ggx_pdf_visible(distr, wis, m);
#endif
            if (microfacetPDF == 0) return f3s(0.0f);
            pdf = microfacetPDF;
            float cosThetaT;
            const float F = fresnel_dielectric_ext(dot3(wi, m), cosThetaT, m_eta);
            F3 weight = f3s(1.0f);
            bool sampleReflection = true;
            if (ppg_rand(key, dim++) > F) { sampleReflection = false; pdf *= 1 - F; }  // bRec.sampler->next1D(), roughdielectric.cpp:553
            else pdf *= F;
            float dwh_dwo;
            if (sampleReflection) {
                wo = m * (2 * dot3(wi, m)) - wi;
                if (wi.z * wo.z <= 0) return f3s(0.0f);
                weight = mul3(weight, M.refl);
                dwh_dwo = 1.0f / (4.0f * dot3(wo, m));
            } else {
                if (cosThetaT == 0) return f3s(0.0f);
                float e2 = m_eta;  // refract(wi, m, eta, cosThetaT), util.cpp:767-772
                if (cosThetaT < 0) e2 = 1 / e2;
                wo = m * (dot3(wi, m) * e2 + cosThetaT) - wi * e2;
                eta = cosThetaT < 0 ? m_eta : m_invEta;
                if (wi.z * wo.z >= 0) return f3s(0.0f);
                float factor = cosThetaT < 0 ? m_invEta : m_eta;
                weight = mul3(weight, M.spec * (factor * factor));
                float sqrtDenom = dot3(wi, m) + eta * dot3(wo, m);
                dwh_dwo = (eta * eta * dot3(wo, m)) / (sqrtDenom * sqrtDenom);
            }
#if PPG_MFD
            if (distr.sampleAll)  // roughdielectric.cpp:608-611
                weight = weight * ppg_abs(ggx_eval(distr, m) * (ggx_smith_g1(distr, wi, m) * ggx_smith_g1(distr, wo, m)) * dot3(wi, m) / (microfacetPDF * wi.z));
            else
#endif
            weight = weight * ggx_smith_g1(distr, wo, m);
            pdf *= ppg_abs(dwh_dwo);
            return weight;
        }
        case PPG_BSDF_THINDIELECTRIC: {  // thindielectric.cpp:203-232
            const float Rr = thin_R(M, wi.z);
            delta = true;
            if (sx <= Rr) {
                wo = f3(-wi.x, -wi.y, wi.z);
                pdf = Rr;
                return M.refl;
            }
            isnull = true;
            wo = -wi;  // transmit()
            pdf = 1 - Rr;
            return M.spec;
        }
#if PPG_LOBES
        case PPG_BSDF_ROUGHDIFFUSE:  // roughdiffuse.cpp:241-251
            if (wi.z <= 0) return f3s(0.0f);
            wo = cosine_hemisphere(sx, sy);
            pdf = PPG_INV_PI_F * wo.z;
            return div3(roughdiffuse_eval(M.refl, M.alpha, (M.flags & PPG_MAT_FAST_APPROX) != 0, wi, wo), pdf);
        case PPG_BSDF_DIFFTRANS:  // difftrans.cpp:105-116: the hemisphere opposite wi, weight = the transmittance
            wo = cosine_hemisphere(sx, sy);
            if (wi.z > 0) wo.z *= -1;
            pdf = ppg_abs(wo.z) * PPG_INV_PI_F;
            return M.refl;
        case PPG_BSDF_PHONG: {  // phong.cpp:183-240
            if (wi.z <= 0) return f3s(0.0f);  // (its pdf() is 0 there)
            const float w = phong_weight(M);
            const float4 sd = phong_sample_dir(w, M.alpha, wi, sx, sy);
            wo = f3(sd.x, sd.y, sd.z);
            if (sd.w == 0.0f) return f3s(0.0f);
            pdf = phong_pdf(w, M.alpha, wi, wo);
            if (pdf == 0) return f3s(0.0f);
            return div3(phong_eval(M.refl, M.spec, M.alpha, wi, wo), pdf);
        }
#endif
#if PPG_NORMALMAP_NULL
        case PPG_BSDF_NULL:  // null.cpp:63-75: straight through, on either side; eval() and pdf() are 0 for every non-discrete query
            delta = true;
            isnull = true;
            wo = -wi;
            pdf = 1;
            return f3s(1.0f);
#endif
    }
    return f3s(0.0f);
}
#if PPG_COAT
// ------------------------------------------------------------------------------------------------
// The coating / roughcoating adapters (coating.cpp:202-371, roughcoating.cpp:229-451) around mat_*_one: a dielectric layer over the nested
// BSDF, inside the two-sided adapter.  M.coat points at the material's rows of DevScene::coat (layout there).  All type masks are "all
// components", as the integrator asks; the measure is the solid angle, except for a delta sample.
// ------------------------------------------------------------------------------------------------
D bool coat_rough(const Mat &M) { return (__float_as_uint(M.coat[0].w) & PPG_COATF_KIND) == 2u; }
// refractIn (coating.cpp:207-212); refractOut (214-219) is the same function of (invEta, eta)
D F3 coat_refract_in(F3 w, float eta, float invEta, float &R) {
    float cosThetaT;
    R = fresnel_dielectric_ext(ppg_abs(w.z), cosThetaT, eta);
    return f3(invEta * w.x, invEta * w.y, -fsignum(w.z) * cosThetaT);
}
// refractTo (roughcoating.cpp:235-255): invEta = m_invEta towards the interior, m_eta towards the exterior; the zero vector = total
// internal reflection
D F3 coat_refract_to(F3 w, float invEta) {
    const float sinThetaTSqr = invEta * invEta * (1.0f - w.z * w.z);
    if (sinThetaTSqr >= 1.0f) return f3s(0.0f);
    const float cosThetaT = __builtin_sqrtf(1.0f - sinThetaTSqr);
    return f3(invEta * w.x, invEta * w.y, w.z > 0.0f ? cosThetaT : -cosThetaT);
}
// m_roughTransmittance->eval(cosTheta, alpha) on the coat's own slice (rtrans.h:185-196, 233).  The table keeps the slice's distance from
// the nested material's, in rows of ppg_scene.rtrans: Mat carries one slice pointer.
MFD_CALL float coat_rough_T(const float *rt, int rows, int rt_n, float cosTheta) {
    const float warped = dm_pow(ppg_abs(cosTheta), 0.25f);
    if (!(cosTheta >= 0)) return 0.0f;
    return ppg_min(1.0f, ppg_max(0.0f, cubic_interp_1d(warped, rt + (ptrdiff_t)rows * (ptrdiff_t)(rt_n + 1), rt_n)));
}
D float coat_T(const Mat &M, float cosTheta) { return coat_rough_T(M.rt, __float_as_int(M.coat[2].w), M.rt_n, cosTheta); }
D Mfd coat_mfd(const Mat &M) {  // MicrofacetDistribution(m_type, alpha, m_sampleVisible), microfacet.h:67-93
    const unsigned int bits = __float_as_uint(M.coat[0].w);
    Mfd d;
    d.type = (int)((bits >> PPG_COATF_TYPE_SHIFT) & 3u);
    d.alphaU = d.alphaV = ppg_max(M.coat[1].w, 1e-4f);
    d.sampleAll = (bits & PPG_COATF_SAMPLE_ALL) != 0u;
    d.exponentU = 0.0f; d.exponentV = 0.0f;
    if (d.type == MFD_PHONG) mfd_phong_exponent(d);
    return d;
}
// the reallocated probability of the coat's own component (coating.cpp:270-272, roughcoating.cpp:346-348)
D float coat_prob_specular(float p, float w) { return (p * w) / (p * w + (1 - p) * (1 - w)); }
// exp(-sigmaA * thickness * (1/|cos i'| + 1/|cos o'|)) (coating.cpp:243-247)
D F3 coat_absorb(const Mat &M, F3 r, float cosI, float cosO) {
    const float4 c1 = M.coat[1];
    const F3 sigmaA = f3(c1.x, c1.y, c1.z) * M.coat[0].y;
    if (iszero3(sigmaA)) return r;
    const float t = 1 / ppg_abs(cosI) + 1 / ppg_abs(cosO);
    return mul3(r, f3(dm_exp(-sigmaA.x * t), dm_exp(-sigmaA.y * t), dm_exp(-sigmaA.z * t)));
}
MFD_CALL F3 coat_eval(Mat M, F3 wi, F3 wo) {  // coating.cpp:221-258, roughcoating.cpp:257-318
    const float eta = M.coat[0].x, invEta = 1 / eta;
    F3 result = f3s(0.0f), wiP, woP;
    float a, b;
    if (!coat_rough(M)) {
        wiP = coat_refract_in(wi, eta, invEta, a);
        woP = coat_refract_in(wo, eta, invEta, b);
        if (a == 1 || b == 1) return result;
        a = 1 - a; b = 1 - b;
    } else {
        if (wo.z * wi.z > 0) {
            const Mfd distr = coat_mfd(M);
            const F3 H = norm3(wo + wi) * fsignum(wo.z);
            const float Dm = ggx_eval(distr, H);
            const float F = fresnel_dielectric_ext(ppg_abs(dot3(wi, H)), eta);
            const float G = ggx_smith_g1(distr, wi, H) * ggx_smith_g1(distr, wo, H);
            const float value = F * Dm * G / (4.0f * ppg_abs(wi.z));
            const float4 c2 = M.coat[2];
            result = f3(c2.x, c2.y, c2.z) * value;
        }
        wiP = coat_refract_to(wi, invEta);
        woP = coat_refract_to(wo, invEta);
        if (iszero3(wiP) || iszero3(woP)) return result;  // (only a layer with eta < 1 gets here)
        a = coat_T(M, ppg_abs(wi.z)); b = coat_T(M, ppg_abs(wo.z));
    }
    F3 nested = MAT_EVAL_ONE(M, wiP, woP) * a * b;
    nested = coat_absorb(M, nested, wiP.z, woP.z);
    nested = nested * (invEta * invEta * wo.z / woP.z);
    return result + nested;
}
MFD_CALL float coat_pdf(Mat M, F3 wi, F3 wo) {  // coating.cpp:260-296, roughcoating.cpp:320-382
    const float4 c0 = M.coat[0];
    const float eta = c0.x, invEta = 1 / eta;
    float result = 0.0f, probSpecular;
    F3 wiP, woP;
    if (!coat_rough(M)) {
        float R12, R21;
        wiP = coat_refract_in(wi, eta, invEta, R12);
        probSpecular = coat_prob_specular(R12, c0.z);
        woP = coat_refract_in(wo, eta, invEta, R21);
        if (R12 == 1 || R21 == 1) return 0.0f;
    } else {
        const F3 H = norm3(wo + wi) * fsignum(wo.z);
        probSpecular = coat_prob_specular(1 - coat_T(M, ppg_abs(wi.z)), c0.z);
        if (wo.z * wi.z > 0) {
            const Mfd distr = coat_mfd(M);
            const float dwh_dwo = 1.0f / (4.0f * ppg_abs(dot3(wo, H)));
            const float prob = mfd_pdf(distr, wi, H);
            result = prob * dwh_dwo * probSpecular;
        }
        wiP = coat_refract_to(wi, invEta);
        woP = coat_refract_to(wo, invEta);
        if (iszero3(wiP) || iszero3(woP)) return result;
    }
    float prob = MAT_PDF_ONE(M, wiP, woP);
    prob *= invEta * invEta * wo.z / woP.z;
    return result + prob * (1 - probSpecular);
}
// sample(), the part before the nested sample() (coating.cpp:298-339, roughcoating.cpp:384-433).  Returns what is left to do:
enum { COAT_NESTED = 1,       // the nested lobes of a coating were chosen: sample the nested BSDF at wiN, then coat_sample_post
       COAT_NESTED_ROUGH = 2, // ... of a roughcoating
       COAT_DONE = 3,         // `result` is final
       COAT_REEVAL = 4 };     // a roughcoating's own lobe was sampled: wo is set, pdf() and eval() / pdf remain
D int coat_sample_pre(const Mat &M, F3 wi, float &sx, float &sy, F3 &wiN, float &ps, float &R12, F3 &result, F3 &wo, float &pdf, bool &delta,
                      float &eta, bool &isnull) {
    const float4 c0 = M.coat[0];
    const float m_eta = c0.x, m_invEta = 1 / m_eta;
    delta = false; eta = 1.0f; pdf = 0.0f; wo = f3s(0.0f); isnull = false;
    result = f3s(0.0f);
    if (!coat_rough(M)) {
        wiN = coat_refract_in(wi, m_eta, m_invEta, R12);
        ps = coat_prob_specular(R12, c0.z);
        if (sx < ps) {
            sx /= ps;  // (as the reference does; nothing reads it)
            wo = f3(-wi.x, -wi.y, wi.z);
            delta = true;
            pdf = ps;
            const float4 c2 = M.coat[2];
            result = f3(c2.x, c2.y, c2.z) * (R12 / pdf);
            return COAT_DONE;
        }
        sx = (sx - ps) / (1 - ps);
        if (R12 == 1.0f) return COAT_DONE;
        return COAT_NESTED;
    }
    ps = coat_prob_specular(1 - coat_T(M, ppg_abs(wi.z)), c0.z);
    if (sy < ps) {
        sy /= ps;
        const float4 ms = mfd_sample(coat_mfd(M), wi, sx, sy);
        const F3 m = f3(ms.x, ms.y, ms.z);
        wo = m * (2 * dot3(wi, m)) - wi;
        if (wo.z * wi.z <= 0) { wo = f3s(0.0f); return COAT_DONE; }
        return COAT_REEVAL;
    }
    sy = (sy - ps) / (1 - ps);
    wiN = coat_refract_to(wi, m_invEta);
    if (iszero3(wiN)) return COAT_DONE;
    return COAT_NESTED_ROUGH;
}
// ... and the part after it (coating.cpp:340-370, roughcoating.cpp:434-441): wo, pdf, delta are the nested sample's
D int coat_sample_post(const Mat &M, int state, F3 wiN, float ps, float R12, F3 &result, F3 &wo, float &pdf, bool delta) {
    const float m_eta = M.coat[0].x, m_invEta = 1 / m_eta;
    if (iszero3(result)) { result = f3s(0.0f); wo = f3s(0.0f); pdf = 0.0f; return COAT_DONE; }
    const F3 woP = wo;
    if (state == COAT_NESTED_ROUGH) {
        wo = coat_refract_to(woP, m_eta);
        if (iszero3(wo)) { result = f3s(0.0f); pdf = 0.0f; return COAT_DONE; }
        return COAT_REEVAL;
    }
    result = coat_absorb(M, result, wiN.z, woP.z);
    float R21;
    wo = coat_refract_in(woP, m_invEta, m_eta, R21);  // refractOut
    if (R21 == 1.0f) { result = f3s(0.0f); wo = f3s(0.0f); pdf = 0.0f; return COAT_DONE; }
    pdf *= 1.0f - ps;
    result = div3(result, 1.0f - ps);
    result = result * ((1 - R12) * (1 - R21));
    if (!delta) pdf *= m_invEta * m_invEta * wo.z / woP.z;
    return COAT_DONE;
}
#endif
#if PPG_BLEND
// ------------------------------------------------------------------------------------------------
// The blendbsdf / mixturebsdf combinators (blendbsdf.cpp:135-275, mixturebsdf.cpp:174-282) over mat_*_one, where a coat sits: inside the
// two-sided adapter.  M.blend points at the material's 16 words of DevScene::blend (layout there); ppg_set_scene has checked every child
// index and that no child is itself blended, coated or wrapped, so the loops below are bounded by PPG_BLEND_MAX and nothing recurses.  One
// child's Mat is live at a time: it is loaded — record, bitmaps at the hit's uv, microfacet entry —, used and dropped.
// ------------------------------------------------------------------------------------------------
#define MAT_SCENE_PARAM , const DevScene &S
#define MAT_SCENE_ARG , S
D bool blend_is_mixture(const float *b) { return (__float_as_uint(b[PPG_BLENDW_BITS]) & PPG_BLENDF_KIND) == 2u; }
D int blend_n(const float *b) { return (int)((__float_as_uint(b[PPG_BLENDW_BITS]) >> PPG_BLENDF_N_SHIFT) & 7u); }
// blendbsdf's weight: min(1, max(0, m_weight->eval(its).average())) (blendbsdf.cpp:136-137); a constant was clamped by ppg_set_scene
D float blend_w(const DevScene &S, const Mat &M) {
    const unsigned int tw = __float_as_uint(M.blend[PPG_BLENDW_TEX]);
    float w = M.blend[PPG_BLENDW_WEIGHT + 1];
    if (tw) { const float4 t = tex_eval_slot(S.textures, tw, M.bu, M.bv); w = avg3(f3(t.x, t.y, t.z)); }
    return ppg_min(1.0f, ppg_max(0.0f, w));
}
// child i's factor in eval() and in pdf(): blend (1 - w, w) for both; mixture m_weights[i] and m_pdf[i] = cdf[i + 1] - cdf[i] (pmf.h:100)
D void blend_weight(const float *b, bool mix, float w1, int i, float &we, float &wp) {
    if (mix) { we = b[PPG_BLENDW_WEIGHT + i]; wp = b[PPG_BLENDW_CDF + i + 1] - b[PPG_BLENDW_CDF + i]; }
    else { we = i == 0 ? 1 - w1 : w1; wp = we; }
}
D Mat blend_child(const DevScene &S, const Mat &M, int i) {
    const int id = __float_as_int(M.blend[PPG_BLENDW_CHILD + i]);
    Mat C = load_material(S, id);
    const unsigned int tex = __float_as_uint(S.materials[PPG_MAT_STRIDE * (size_t)id + 5].x) & 0xffffu;
    if (tex) { const float4 t = tex_eval_slot(S.textures, tex, M.bu, M.bv); C.refl = f3(t.x, t.y, t.z); }
    mat_apply_textures(S, id, M.bu, M.bv, C);
    mat_apply_mfd_textures(S, id, M.bu, M.bv, C);
    return C;
}
// eval() / pdf() of a child under the discrete measure, which a blend asks of the children it did not sample after a delta sample:
// conductor.cpp:223-252, plastic.cpp:245-307 (the mirror-direction test against DeltaEpsilon = 1e-3); every other child answers 0
D float mat_mirror_error(F3 wi, F3 wo) { return ppg_abs(dot3(f3(-wi.x, -wi.y, wi.z), wo) - 1); }
D F3 mat_eval_one_discrete(const Mat &C, F3 wi, F3 wo) {
    if (C.type == PPG_BSDF_MIRROR || C.type == PPG_BSDF_CONDUCTOR) {
        if (wi.z <= 0 || wo.z <= 0 || mat_mirror_error(wi, wo) > 1e-3f) return f3s(0.0f);
        return mul3(C.refl, fresnel_conductor_exact(wi.z, C.eta, C.k));
    }
    if (C.type == PPG_BSDF_PLASTIC) {
        if (wo.z <= 0 || wi.z <= 0) return f3s(0.0f);
        const float Fi = fresnel_dielectric_ext(wi.z, C.eta.x);
        if (mat_mirror_error(wi, wo) < 1e-3f) return C.spec * Fi;
    }
    return f3s(0.0f);
}
D float mat_pdf_one_discrete(const Mat &C, F3 wi, F3 wo) {
    if (C.type == PPG_BSDF_MIRROR || C.type == PPG_BSDF_CONDUCTOR) {
        if (wi.z <= 0 || wo.z <= 0 || mat_mirror_error(wi, wo) > 1e-3f) return 0.0f;
        return 1.0f;
    }
    if (C.type == PPG_BSDF_PLASTIC) {
        if (wo.z <= 0 || wi.z <= 0) return 0.0f;
        const float Fi = fresnel_dielectric_ext(wi.z, C.eta.x);
        if (mat_mirror_error(wi, wo) < 1e-3f) return plastic_prob_specular(C, Fi);
    }
    return 0.0f;
}
D F3 blend_eval(const DevScene &S, const Mat &M, F3 wi, F3 wo) {  // blendbsdf.cpp:139-142, mixturebsdf.cpp:177-179
    const float *b = M.blend;
    const bool mix = blend_is_mixture(b);
    const int n = blend_n(b);
    const float w1 = mix ? 0.0f : blend_w(S, M);
    F3 result = f3s(0.0f);
#pragma unroll 1
    for (int i = 0; i < n && i < PPG_BLEND_MAX; ++i) {
        float we, wp;
        blend_weight(b, mix, w1, i, we, wp);
        const Mat C = blend_child(S, M, i);
        result = result + MAT_EVAL_ONE(C, wi, wo) * we;
    }
    return result;
}
D float blend_pdf(const DevScene &S, const Mat &M, F3 wi, F3 wo) {  // blendbsdf.cpp:160-163, mixturebsdf.cpp:194-196
    const float *b = M.blend;
    const bool mix = blend_is_mixture(b);
    const int n = blend_n(b);
    const float w1 = mix ? 0.0f : blend_w(S, M);
    float result = 0.0f;
#pragma unroll 1
    for (int i = 0; i < n && i < PPG_BLEND_MAX; ++i) {
        float we, wp;
        blend_weight(b, mix, w1, i, we, wp);
        const Mat C = blend_child(S, M, i);
        result += MAT_PDF_ONE(C, wi, wo) * wp;
    }
    return result;
}
// sample(), the part before the chosen child's sample() (blendbsdf.cpp:229-235, mixturebsdf.cpp:248 with sampleReuse, pmf.h:183-188): the
// child, the reused sample, and the child's factors in eval() and pdf()
D int blend_sample_pre(const DevScene &S, const Mat &M, float &sx, float &w1, float &we, float &wp) {
    const float *b = M.blend;
    const bool mix = blend_is_mixture(b);
    int entry;
    w1 = 0.0f;
    if (!mix) {
        w1 = blend_w(S, M);
        const float w0 = 1 - w1;
        if (sx < w0) { entry = 0; sx /= w0; }
        else { entry = 1; sx = (sx - w0) / w1; }
    } else {
        entry = pmf_sample(b + PPG_BLENDW_CDF, blend_n(b) + 1, sx);
        // (a sample of 1 or more — none comes from the sampler — would walk past a last child of weight 0: the index stays in the table)
        const int last = (blend_n(b) < PPG_BLEND_MAX ? blend_n(b) : PPG_BLEND_MAX) - 1;
        if (entry > last) entry = last;
        if (entry < 0) entry = 0;
        const float c0 = b[PPG_BLENDW_CDF + entry], c1 = b[PPG_BLENDW_CDF + entry + 1];
        sx = (sx - c0) / (c1 - c0);
    }
    blend_weight(b, mix, w1, entry, we, wp);
    return entry;
}
// ... and the part after it (blendbsdf.cpp:237-253, mixturebsdf.cpp:250-266): the other children's pdf() and eval() in the measure of
// what was sampled.  A sum that is not a positive finite density is a failed sample, where the reference would divide by it.
D F3 blend_sample_post(const DevScene &S, const Mat &M, int entry, float w1, float we, float wp, F3 wi, F3 result, F3 &wo, float &pdf, bool &delta) {
    const float *b = M.blend;
    const bool mix = blend_is_mixture(b);
    const int n = blend_n(b);
    if (iszero3(result)) { wo = f3s(0.0f); pdf = 0.0f; delta = false; return f3s(0.0f); }
    result = result * (we * pdf);
    pdf *= wp;
#pragma unroll 1
    for (int i = 0; i < n && i < PPG_BLEND_MAX; ++i) {
        if (i == entry) continue;
        float wei, wpi;
        blend_weight(b, mix, w1, i, wei, wpi);
        const Mat C = blend_child(S, M, i);
        if (delta) {
            pdf += mat_pdf_one_discrete(C, wi, wo) * wpi;
            result = result + mat_eval_one_discrete(C, wi, wo) * wei;
        } else {
            pdf += MAT_PDF_ONE(C, wi, wo) * wpi;
            result = result + MAT_EVAL_ONE(C, wi, wo) * wei;
        }
    }
    if (!(pdf > 0) || !ppg_isfinite(pdf)) { wo = f3s(0.0f); pdf = 0.0f; delta = false; return f3s(0.0f); }
    return div3(result, pdf);
}
#else
#define MAT_SCENE_PARAM
#define MAT_SCENE_ARG
#endif
// + the TwoSided adapter (twosided.cpp:120-180) and, outside it, the Mask adapter (mask.cpp:108-214).  (MAT_SCENE_PARAM: the blend family's
// functions also take the scene, whose tables a blended material's children are read from.)
D F3 mat_eval(const Mat &M, F3 wi, F3 wo MAT_SCENE_PARAM) {
    if (mat_two_sided(M) && !(wi.z > 0)) { wi.z *= -1; wo.z *= -1; }
#if PPG_BLEND
    F3 r = M.blend ? blend_eval(S, M, wi, wo) : (M.coat ? coat_eval(M, wi, wo) : MAT_EVAL_ONE(M, wi, wo));
#elif PPG_COAT
    F3 r = M.coat ? coat_eval(M, wi, wo) : MAT_EVAL_ONE(M, wi, wo);
#else
    F3 r = mat_eval_one(M, wi, wo);
#endif
    return mat_masked(M) ? mul3(r, M.opacity) : r;
}
D float mat_pdf(const Mat &M, F3 wi, F3 wo MAT_SCENE_PARAM) {
    if (mat_two_sided(M) && !(wi.z > 0)) { wi.z *= -1; wo.z *= -1; }
#if PPG_BLEND
    float r = M.blend ? blend_pdf(S, M, wi, wo) : (M.coat ? coat_pdf(M, wi, wo) : MAT_PDF_ONE(M, wi, wo));
#elif PPG_COAT
    float r = M.coat ? coat_pdf(M, wi, wo) : MAT_PDF_ONE(M, wi, wo);
#else
    float r = mat_pdf_one(M, wi, wo);
#endif
    return mat_masked(M) ? r * lum3(M.opacity) : r;
}
D F3 mat_sample_ts(const Mat &M, F3 wi, float sx, float sy, F3 &wo, float &pdf, bool &delta, float &eta, bool &isnull, unsigned int key,
                   unsigned int &dim MAT_SCENE_PARAM);
// key / dim: the path's sampler, for plug-ins whose sample() draws from it (roughdielectric)
D F3 mat_sample(const Mat &M, F3 wi, float sx, float sy, F3 &wo, float &pdf, bool &delta, float &eta, bool &isnull, unsigned int key,
                unsigned int &dim MAT_SCENE_PARAM) {
    // (ONE call of the nested BSDF's sample(): see the note on code size in shade_one)
    const bool masked = mat_masked(M);
    const float prob = masked ? lum3(M.opacity) : 1.0f;
    if (masked && !(sx < prob)) {
        wo = -wi;
        eta = 1.0f;
        delta = true;
        isnull = true;
        pdf = 1 - prob;
        return div3(f3s(1.0f) - M.opacity, pdf);
    }
    if (masked) sx /= prob;
    F3 result = mat_sample_ts(M, wi, sx, sy, wo, pdf, delta, eta, isnull, key, dim MAT_SCENE_ARG);
    if (masked) {
        result = div3(mul3(result, M.opacity), prob);
        pdf *= prob;
    }
    return result;
}
#if PPG_BLEND
D F3 mat_sample_ts(const Mat &M0, F3 wi, float sx, float sy, F3 &wo, float &pdf, bool &delta, float &eta, bool &isnull, unsigned int key,
                   unsigned int &dim MAT_SCENE_PARAM) {
    bool flipped = false;
    if (mat_two_sided(M0) && wi.z < 0) { wi.z *= -1; flipped = true; }
    // (a blend chooses the child whose sample() runs — still the ONE call below — and adds the other children afterwards)
    Mat M = M0;
    int entry = 0;
    float bw1 = 0.0f, bwe = 1.0f, bwp = 1.0f;
    if (M0.blend) { entry = blend_sample_pre(S, M0, sx, bw1, bwe, bwp); M = blend_child(S, M0, entry); }
#else
D F3 mat_sample_ts(const Mat &M, F3 wi, float sx, float sy, F3 &wo, float &pdf, bool &delta, float &eta, bool &isnull, unsigned int key,
                   unsigned int &dim) {
    bool flipped = false;
    if (mat_two_sided(M) && wi.z < 0) { wi.z *= -1; flipped = true; }
#endif
#if PPG_COAT
    // (still ONE call of the nested sample(): a coat only changes its arguments before and its results after)
    F3 result, wiN = wi;
    float ps = 0.0f, R12 = 0.0f;
    int coat = 0;
    if (M.coat) coat = coat_sample_pre(M, wi, sx, sy, wiN, ps, R12, result, wo, pdf, delta, eta, isnull);
    if (coat < COAT_DONE) {
        result = mat_sample_one(M, wiN, sx, sy, wo, pdf, delta, eta, isnull, key, dim);
        if (coat) coat = coat_sample_post(M, coat, wiN, ps, R12, result, wo, pdf, delta);
    }
    if (coat == COAT_REEVAL) {  // roughcoating.cpp:443-450
        pdf = coat_pdf(M, wi, wo);
        if (pdf != 0) result = div3(coat_eval(M, wi, wo), pdf);
        // (not finite: the layer's own lobe sampled from below a one-sided surface, where the visible normals of a direction under the
        // horizon mean nothing — a failed sample, where the reference would hand its caller the NaN)
        if (pdf == 0 || !ppg_isfinite(pdf) || !ppg_isfinite(result.x + result.y + result.z) || !ppg_isfinite(wo.x + wo.y + wo.z)) {
            result = f3s(0.0f); wo = f3s(0.0f); pdf = 0.0f;
        }
    }
#else
    F3 result = mat_sample_one(M, wi, sx, sy, wo, pdf, delta, eta, isnull, key, dim);
#endif
#if PPG_BLEND
    if (M0.blend) result = blend_sample_post(S, M0, entry, bw1, bwe, bwp, wi, result, wo, pdf, delta);
#endif
    if (flipped && !iszero3(result) && pdf != 0) wo.z *= -1;
    return result;
}

// ------------------------------------------------------------------------------------------------
// SD-tree
// ------------------------------------------------------------------------------------------------
struct __attribute__((aligned(32))) SNode {  // sampling quadtree node, 32 B
    float sum[4];
    unsigned short child[4];
    unsigned int pad[2];
};

struct __attribute__((aligned(16))) LeafHdr {  // one per S-tree node, 64 B
    unsigned int s_base, s_num;  // sampling D-tree: first node in the SNode pool, node count
    float s_sum, s_statw;        // DTree::m_atomic {sum, statisticalWeight} of the sampling tree (GP:538-557)
    unsigned int b_base, b_num;  // building D-tree block in bchild / bacc
    int s_depth, b_depth;        // m_maxDepth
    float theta;                 // AdamOptimizer::State (GP:116-124)
    int adam_iter;
    float adam_m, adam_v;
    float b_statw;               // statisticalWeightBuilding() as float (valid after build; halved by refine)
    float adam_bg, adam_ba;      // AdamOptimizer::State::batchGradient / batchAccumulation (GP:121-122): the partial batch of append()
    unsigned int pad;
};

// One deferred DTreeWrapper::optimizeBsdfSamplingFraction call (= ppg_adam_record of include/ppg.h)
struct __attribute__((aligned(16))) AdamRec {
    unsigned long long key;  // leaf << PPG_ADAM_LEAF_SHIFT | path << PPG_ADAM_CODE_BITS | code
    float product, woPdf, bsdfPdf, dTreePdf, weight, pad;
};

struct DevTree {
    const int4 *stree;            // {axis, child0, child1, -}
    LeafHdr *hdr;                 // per S-tree node
    const SNode *snodes;          // sampling pool
    const ushort4 *bchild;        // building pool topology
    unsigned long long *bacc;     // building pool accumulators [node*4 + slot], 2^-24 fixed point
    unsigned long long *bweight;  // per S-tree node: building statistical weight accumulator (folded, see *_rep)
    // Records of the round for the sampling-fraction optimiser (include/ppg.h "Learning the BSDF sampling fraction"): written at
    // position adam_base[path] + vertex when adam_base != nullptr (every record's place is known in advance: nearest / stochastic
    // spatial filter without next-event estimation — the buffer is then already ordered by (path, code) and only a stable sort
    // by leaf remains), otherwise appended through adam_count[0] (adam_count[1] = overflow flag) and sorted by the whole key.
    unsigned long long *adam_keys;
    AdamRec *adam_recs;
    unsigned int *adam_count;
    const unsigned int *adam_base;
    unsigned int adam_cap;
    // Replicated accumulation targets [node * PPG_REPLICAS + r]: a popular S-tree leaf receives several percent of all
    // records of a pass and one address sustains only ~90 atomics/µs; workgroups spread over the replicas,
    // k_fold_replicas adds them into the compact arrays above (integer sums: exact).
    unsigned long long *bweight_rep;
    float aabb_min[3], aabb_ext[3];  // cubified AABB (GP:857-859)
    float aabb_max[3];
    int is_built;
    // Lookup accelerator: the S-tree cycles its split axis x,y,z, so the first 3*GRID_BITS levels of any descent
    // are determined by the top GRID_BITS bits of each normalised coordinate.  grid[cell] = node reached after
    // min(3*GRID_BITS, depth of the leaf) levels | levels << 27.  One read replaces up to 18 dependent ones.
    const unsigned int *grid;
    // The optimiser's variable per S-tree node as it was when the round began (nullptr: read it in the leaf header).  A round's stragglers are
    // finished BESIDE the application of that round's records and the next round's (ppg_hip.hip "Stragglers"), which rewrite the headers;
    // they must go on sampling with the fractions of their own round (include/ppg.h: all paths of a round see the fractions in effect at its start).
    const float *theta_frozen;
};
#define PPG_REPLICAS 32
#define PPG_GRID_BITS 6
#define PPG_GRID_DIM (1 << PPG_GRID_BITS)
#define PPG_GRID_LEVELS (3 * PPG_GRID_BITS)

// STree::dTreeWrapper (GP:897-905) + STreeNode::dTreeWrapper (GP:761-769): leaf index and voxel size.
// The reference halves p[axis] / size[axis] level by level; every one of those operations is exact in
// binary floating point (×2, −0.5 on [0.5,1), ÷2), so jumping 18 levels through the grid and computing
// the voxel size as extent · 2^-n gives bit-identical results (tests compare against the literal descent
// of the oracle).
D int stree_lookup(const DevTree &T, F3 pw, F3 &size) {
    size = f3(T.aabb_ext[0], T.aabb_ext[1], T.aabb_ext[2]);
    float p[3];
    p[0] = (pw.x - T.aabb_min[0]) / size.x;
    p[1] = (pw.y - T.aabb_min[1]) / size.y;
    p[2] = (pw.z - T.aabb_min[2]) / size.z;
    int cell[3];
    float rem[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float s = p[a] * (float)PPG_GRID_DIM;
        int c = (s < (float)PPG_GRID_DIM) ? ((s < 0.0f) ? 0 : (int)s) : (PPG_GRID_DIM - 1);  // out-of-cube points follow child 0 / child 1 forever
        cell[a] = c;
        rem[a] = s - (float)c;
    }
    const unsigned int e = T.grid[(cell[2] * PPG_GRID_DIM + cell[1]) * PPG_GRID_DIM + cell[0]];
    int idx = (int)(e & 0x07ffffffu);
    int depth = (int)(e >> 27);
    if (depth == PPG_GRID_LEVELS) {  // possibly deeper than the grid: continue the literal descent on the remainders
        for (;;) {
            int4 n = T.stree[idx];
            if (n.y == 0) break;
            int a = n.x;
            ++depth;
            if (rem[a] < 0.5f) {
                rem[a] *= 2;
                idx = n.y;
            } else {
                rem[a] = (rem[a] - 0.5f) * 2;
                idx = n.z;
            }
        }
    }
    // levels along x, y, z of a leaf at depth D (root splits x, then y, z, x, ...)
    size = f3(size.x * ppg_exp2i(-((depth + 2) / 3)), size.y * ppg_exp2i(-((depth + 1) / 3)), size.z * ppg_exp2i(-(depth / 3)));
    return idx;
}

// DTreeWrapper::canonicalToDir / dirToCanonical (GP:586-608)
D F3 canonical_to_dir(float px, float py) {
    const float cosTheta = 2 * px - 1;
    const float phi = 2 * PPG_PI_F * py;
    const float sinTheta = __builtin_sqrtf(1 - cosTheta * cosTheta);
    float sinPhi, cosPhi;
    dm_sincos(phi, &sinPhi, &cosPhi);
    return f3(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta);
}
D void dir_to_canonical(F3 d, float &px, float &py) {
    if (!ppg_isfinite(d.x) || !ppg_isfinite(d.y) || !ppg_isfinite(d.z)) { px = 0; py = 0; return; }
    const float cosTheta = ppg_min(ppg_max(d.z, -1.0f), 1.0f);
    float phi = dm_atan2(d.y, d.x);
    while (phi < 0) phi = (float)((double)phi + 2.0 * (double)PPG_PI_F);
    px = (cosTheta + 1) / 2;
    py = phi / (2 * PPG_PI_F);
}

// QuadTreeNode::childIndex (GP:205-217)
D int quad_child_index(float &px, float &py) {
    int res = 0;
    if (px < 0.5f) px *= 2; else { px = (px - 0.5f) * 2; res |= 1; }
    if (py < 0.5f) py *= 2; else { py = (py - 0.5f) * 2; res |= 2; }
    return res;
}

// One sampling node in registers: sums as float4, children as packed u16x4.  Dynamic indexing of a struct
// would send it through LDS/scratch and serialise its two 16-byte loads; selects keep it in VGPRs.
struct NodeR {
    float4 s;
    uint2 c;
};
D NodeR load_node(const SNode *p) {
    NodeR n;
    const float4 *q = reinterpret_cast<const float4 *>(p);
    n.s = q[0];
    float4 t = q[1];
    n.c = make_uint2(__float_as_uint(t.x), __float_as_uint(t.y));
    return n;
}
D float node_sum(const NodeR &n, int i) { return i == 0 ? n.s.x : (i == 1 ? n.s.y : (i == 2 ? n.s.z : n.s.w)); }
D unsigned int node_child(const NodeR &n, int i) {
    unsigned int w = (i & 2) ? n.c.y : n.c.x;
    return (i & 1) ? (w >> 16) : (w & 0xffffu);
}

// DTree::mean (GP:387-393)
D float dtree_mean(float sum, float statw) {
    if (statw == 0) return 0;
    const float factor = 1 / (PPG_PI_F * 4 * statw);
    return factor * sum;
}

// what sampling / pdf evaluation need of a leaf's header
struct DTreeRef {
    unsigned int s_base;
    float s_sum, s_statw;
};
D DTreeRef dtree_ref(const LeafHdr &h) { DTreeRef r; r.s_base = h.s_base; r.s_sum = h.s_sum; r.s_statw = h.s_statw; return r; }

// DTree::pdf + QuadTreeNode::pdf (GP:415-421, 232-245), iterative
template <typename Stack>
D float dtree_pdf(const DevTree &T, const DTreeRef &h, float px, float py, Stack factors) {
    if (!(dtree_mean(h.s_sum, h.s_statw) > 0)) return 1 / (4 * PPG_PI_F);
    // the recursion multiplies factors from the leaf upwards: f1 * (f2 * (f3 * ...)); keep that order
    int nf = 0;
    unsigned int node = 0;
    float result;
    for (;;) {
        const NodeR n = load_node(T.snodes + h.s_base + node);
        const int index = quad_child_index(px, py);
        const float si = node_sum(n, index);
        if (!(si > 0)) { result = 0; break; }
        const float factor = 4 * si / (n.s.x + n.s.y + n.s.z + n.s.w);
        const unsigned int c = node_child(n, index);
        if (c == 0) { result = factor; break; }
        factors[nf++] = factor;
        node = c;
    }
    for (int i = nf - 1; i >= 0; --i) result = factors[i] * result;
    return result / (4 * PPG_PI_F);
}

// DTree::sample + QuadTreeNode::sample (GP:431-442, 257-301), iterative.
// The recursion returns origin + 0.5 * child.sample(); unrolled as a stack of origins.
D void dtree_sample(const DevTree &T, const DTreeRef &h, uint32_t key, uint32_t &dim, float &ox, float &oy) {
    if (!(dtree_mean(h.s_sum, h.s_statw) > 0)) {
        ox = ppg_rand(key, dim++);
        oy = ppg_rand(key, dim++);
        return;
    }
    unsigned int orgx = 0, orgy = 0;  // origin.x / origin.y of level i is 0.5 iff bit i is set (GP:271, 282, 291)
    int depth = 0;
    unsigned int node = 0;
    float rx, ry;
    for (;;) {
        const NodeR n = load_node(T.snodes + h.s_base + node);
        int index = 0;
        float topLeft = n.s.x;
        float topRight = n.s.y;
        float partial = topLeft + n.s.z;
        float total = partial + topRight + n.s.w;
        if (!(total > 0.0f)) {
            rx = ppg_rand(key, dim++);
            ry = ppg_rand(key, dim++);
            break;
        }
        float boundary = partial / total;
        float ogx = 0.0f, ogy = 0.0f;
        float sample = ppg_rand(key, dim++);
        if (sample < boundary) {
            sample /= boundary;
            boundary = topLeft / partial;
        } else {
            partial = total - partial;
            ogx = 0.5f;
            sample = (sample - boundary) / (1.0f - boundary);
            boundary = topRight / partial;
            index |= 1 << 0;
        }
        if (sample < boundary) {
            sample /= boundary;
        } else {
            ogy = 0.5f;
            sample = (sample - boundary) / (1.0f - boundary);
            index |= 1 << 1;
        }
        if (ogx != 0.0f) orgx |= 1u << depth;
        if (ogy != 0.0f) orgy |= 1u << depth;
        ++depth;
        const unsigned int c = node_child(n, index);
        if (c == 0) {
            rx = ppg_rand(key, dim++);
            ry = ppg_rand(key, dim++);
            break;
        }
        node = c;
    }
    for (int i = depth - 1; i >= 0; --i) {
        rx = (((orgx >> i) & 1u) ? 0.5f : 0.0f) + 0.5f * rx;
        ry = (((orgy >> i) & 1u) ? 0.5f : 0.0f) + 0.5f * ry;
    }
    ox = ppg_min(ppg_max(rx, 0.0f), 1.0f);
    oy = ppg_min(ppg_max(ry, 0.0f), 1.0f);
}

// per-thread column of a [depth][threads] LDS array: conflict-free, costs no registers
struct LdsColumn {
    float *base;
    int stride;
    D float &operator[](int i) const { return base[i * stride]; }
};
struct RegColumn {
    float v[24];
    D float &operator[](int i) { return v[i]; }
};

D float logistic(float x) { return 1 / (1 + dm_exp(-x)); }  // GP:64-66

#endif
