/*
 * ppg.h — C-ABI of libppg_hip.so, the MI355X-native GuidedPathTracer hot path.
 *
 * Every entry point replaces a piece of the reference integrator plugin
 * (mitsuba/src/integrators/path/guided_path.cpp, cited as GP:line) or of the Mitsuba Integrator
 * interface it implements (mitsuba/include/mitsuba/render/integrator.h, cited as IH:line).
 * The reference-side binding a Mitsuba maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++/torch types; all pointers are host pointers unless the name says `dev`.
 *   - every function returns PPG_OK (0) or a negative error code; ppg_last_error() gives the text.
 *     No exception crosses this boundary (the reference uses Assert/Log(EError) → throw; GP:1023).
 *   - one context per GPU, driven by one host thread; ppg_cancel() is the only call that may come
 *     from another thread (mirrors Integrator::cancel(), IH:84 / GP:1643-1648).
 *   - the caller owns every buffer it passes in; ppg_set_scene() copies.
 */
#ifndef PPG_H
#define PPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPG_OK 0
#define PPG_ERR_INVALID (-1)   /* bad argument / unknown enum string (reference: Assert(false), GP:1023...) */
#define PPG_ERR_DEVICE (-2)    /* HIP error */
#define PPG_ERR_STATE (-3)     /* call out of order (no scene, render not begun, ...) */
#define PPG_ERR_CANCELLED (-4) /* ppg_cancel() was called; render() returns false in the reference (GP:1584) */
#define PPG_ERR_NOMEM (-5)

typedef struct ppg_ctx ppg_ctx;

/* ------------------------------------------------------------------------------------------------
 * Integrator properties.  Names, meaning and defaults are the reference's:
 *   GuidedPathTracer(const Properties&)      GP:1014-1085
 *   MonteCarloIntegrator(const Properties&)  mitsuba/src/librender/integrator.cpp:190-225
 * String-valued properties stay strings so that an unknown value is rejected exactly where the
 * reference asserts.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_config {
    const char *nee;                      /* "never" | "kickstart" | "always"          GP:1015-1024 (default "never") */
    const char *sampleCombination;        /* "discard" | "automatic" | "inversevar"    GP:1026-1035 (default "automatic") */
    const char *spatialFilter;            /* "nearest" | "stochastic" | "box"          GP:1037-1046 (default "nearest") */
    const char *directionalFilter;        /* "nearest" | "box"                         GP:1048-1055 (default "nearest") */
    const char *bsdfSamplingFractionLoss; /* "none" | "kl" | "var"                     GP:1057-1066 (default "none") */
    int32_t sdTreeMaxMemory;              /* MB, -1 = unlimited                        GP:1068 */
    int32_t sTreeThreshold;               /* 12000                                     GP:1069 */
    float dTreeThreshold;                 /* 0.01                                      GP:1070 */
    float bsdfSamplingFraction;           /* 0.5                                       GP:1071 */
    int32_t sppPerPass;                   /* 4                                         GP:1072 */
    const char *budgetType;               /* "spp" | "seconds" (default "seconds")     GP:1074-1081 */
    float budget;                         /* 300                                       GP:1083 */
    int32_t dumpSDTree;                   /* 0                                         GP:1084 */
    /* MonteCarloIntegrator */
    int32_t rrDepth;                      /* 5   integrator.cpp:192 */
    int32_t maxDepth;                     /* -1  integrator.cpp:197 */
    int32_t strictNormals;                /* 0   integrator.cpp:213 */
    int32_t hideEmitters;                 /* 0   integrator.cpp:218 */
    /* Build-specific (no reference counterpart) */
    uint64_t seed;                        /* key of the counter-based sampler that replaces the per-thread SFMT
                                             streams of samplers/independent.cpp (XML `seed` is ignored there) */
    int32_t device;                       /* HIP device ordinal */
    const char *dumpPrefix;               /* "<dest>" of the "<dest>-NN.sdt" dumps, GP:1192-1195; may be NULL */
} ppg_config;

/* Fills *cfg with the reference defaults listed above. */
void ppg_config_default(ppg_config *cfg);

/* ------------------------------------------------------------------------------------------------
 * Scene: what GuidedPathTracer::render() reaches through `Scene*` (GP:1516-1527, 1784, 1934, 2193),
 * flattened.  Triangles only; per-triangle BSDF and emitter indices.
 * ---------------------------------------------------------------------------------------------- */
enum {
    PPG_BSDF_DIFFUSE = 0,          /* mitsuba/src/bsdfs/diffuse.cpp:110-150 (one-sided Lambertian) */
    PPG_BSDF_TWOSIDED_DIFFUSE = 1, /* = PPG_BSDF_DIFFUSE with PPG_MAT_TWOSIDED (kept for the round-1 callers) */
    PPG_BSDF_MIRROR = 2,           /* conductor.cpp:220-290 with material "none" (eta = 0, k = 1: Fresnel = 1): ideal specular
                                      reflection, reflectance = specularReflectance; a delta BSDF — never guided (GP:1942-1944, 1654) */
    PPG_BSDF_CONDUCTOR = 3,        /* conductor.cpp:220-290: smooth conductor, fresnelConductorExact(eta, k) (util.cpp:739-761) */
    PPG_BSDF_ROUGHCONDUCTOR = 4,   /* roughconductor.cpp:247-415 with an isotropic GGX (or, PPG_MAT_BECKMANN, Beckmann) distribution and visible-normal
                                      sampling (microfacet.h:191-276, 425-540, 645-690): glossy ⇒ smooth ⇒ guided */
    PPG_BSDF_PLASTIC = 5,          /* plastic.cpp:247-455: delta specular coat over a diffuse base — the mixed delta/smooth
                                      case of sampleMat (GP:1672-1676) */
    PPG_BSDF_DIELECTRIC = 6,       /* dielectric.cpp:229-400: smooth glass, delta reflection + delta refraction, tracks eta */
    PPG_BSDF_THINDIELECTRIC = 7    /* thindielectric.cpp:152-252: delta reflection + a NULL (pass-through) component — exercises Li's
                                      null branch (GP:2045-2075) and the look-through of rayIntersectAndLookForEmitter /
                                      evalTransmittance (GP:2184-2245, scene.cpp:619-679) */
    ,
    PPG_BSDF_ROUGHDIELECTRIC = 8   /* roughdielectric.cpp:268-606: microfacet reflection + refraction (GGX / Beckmann, visible normals) — a smooth,
                                      TRANSMISSIVE BSDF: guided on both sides; its sample() draws one extra number from the path's sampler */,
    PPG_BSDF_ROUGHPLASTIC = 9      /* roughplastic.cpp:330-501: rough dielectric coating (GGX / Beckmann, visible normals) over a diffuse base; the
                                      energy balance between the two comes from Mitsuba's precomputed rough-transmittance tables
                                      (data/microfacet/{ggx,beckmann}.dat, rtrans.h), handed over as the per-material slice `ppg_scene.rtrans[material.rtrans]` */
    ,
    /* The three lobes below run on the HIP library only (its sixth kernel family, csrc/ppg_device.h PPG_LOBES); the CPU oracle refuses them. */
    PPG_BSDF_ROUGHDIFFUSE = 10,    /* roughdiffuse.cpp:128-252: Oren-Nayar, the full model or (PPG_MAT_FAST_APPROX) the qualitative one; sigma =
                                      alpha / sqrt(2); cosine-hemisphere sampling, weight = eval / pdf; one-sided, smooth */
    PPG_BSDF_DIFFTRANS = 11,       /* difftrans.cpp:76-116: ideal diffuse TRANSMITTER — a smooth transmissive BSDF, guided on both sides; the
                                      cosine hemisphere on the side opposite wi, weight = transmittance; cannot be two-sided */
    PPG_BSDF_PHONG = 12            /* phong.cpp:122-240: modified Phong, a glossy lobe pow(alpha, exponent) around the mirror direction plus a
                                      diffuse one, chosen by specularSamplingWeight = sAvg / (dAvg + sAvg); weight = eval / pdf of the whole */
    ,
    PPG_BSDF_NULL = 13             /* null.cpp:36-80: the pass-through BSDF, one component ENull | EFrontSide | EBackSide — sample() gives wo = -wi with
                                      weight 1, pdf 1, eta 1; eval() and pdf() are 0 for every non-discrete query.  Not smooth: no D-tree, no
                                      next-event estimation at it; the path takes Li's null branch (GP:2045-2075) and the emitter search and shadow
                                      segments pass through it with transmittance 1.  Its usual use: the invisible carrier of an area emitter.
                                      HIP library only, in the kernel family of the three lobes above */
};
#define PPG_BSDF_LAST PPG_BSDF_ROUGHPLASTIC /* the last type the CPU oracle knows */
#define PPG_BSDF_LAST_HIP PPG_BSDF_NULL     /* the last type the HIP library knows */
enum {
    PPG_MAT_TWOSIDED = 1,          /* wrap the (one-sided) BRDF in twosided.cpp:100-180, same BRDF on both sides */
    PPG_MAT_NONLINEAR = 2,         /* plastic: nonlinear = true (plastic.cpp:164) */
    PPG_MAT_BECKMANN = 8,          /* roughconductor: Beckmann distribution (Mitsuba's default) instead of GGX — microfacet.h:199-205,
                                      487-498, 565-642 (visible-normal sampling by numerical inversion), math.cpp:25-72 (erf, erfinv) */
    PPG_MAT_MASK = 4               /* wrap the BSDF (outside a two-sided adapter, if any) in mask.cpp:108-214 with constant `opacity`: a
                                      smooth/null hybrid — its sampled pass-through is recorded for the sampling-fraction optimiser
                                      (GP:2047-2068) */
    ,
    PPG_MAT_FAST_APPROX = 16,      /* roughdiffuse: useFastApprox = true (roughdiffuse.cpp:159-174); refused on every other type */
    PPG_MAT_NORMALMAP = 32         /* bits 16..31 of `texture` name the RGB normal map of a `normalmap` adapter (normalmap.cpp:47-224) instead of a
                                      bumpmap's displacement texture: n = 2 * texel - 1 in the unperturbed shading frame, NOT flipped towards the
                                      geometric normal as bumpmap.cpp does.  HIP library only (the kernel family of the lobes); refused when that
                                      half of `texture` is 0 */
};
enum { PPG_WRAP_REPEAT = 0, PPG_WRAP_MIRROR = 1, PPG_WRAP_CLAMP = 2, PPG_WRAP_ZERO = 3, PPG_WRAP_ONE = 4 }; /* ReconstructionFilter::EBoundaryCondition, mipmap.h:503-560 */

typedef struct ppg_texture {
    /* A bitmap texture as THIS integrator sees it (textures/bitmap.cpp).  Li fetches the BSDF with its.getBSDF() (GP:1934), not
       getBSDF(ray), so Intersection::computePartials never runs, its.hasUVPartials stays false and Texture2D::eval (texture.cpp:112-121)
       always takes the unfiltered branch: BitmapTexture::eval(uv) (bitmap.cpp:431-452) = MIPMap::evalBilinear(0, uv) (mipmap.h:575-596)
       on the full-resolution image — or evalBox for filterType "nearest" — whatever filterType the scene asks for; bump maps read
       evalGradientBilinear(0, uv) (mipmap.h:601-626).  uv = its.uv * (uscale, vscale) + (uoffset, voffset). */
    uint32_t width, height;
    const float *rgb;          /* [height * width * 3] linear RGB: the image after the loader's gamma / sRGB decoding (bitmap.cpp:182-260),
                                  row 0 = first row of the file; luminance images replicated to three channels */
    float uv_scale[2], uv_offset[2];
    int32_t wrap_u, wrap_v;    /* PPG_WRAP_*: wrapModeU / wrapModeV */
    int32_t nearest;           /* filterType = nearest */
} ppg_texture;


typedef struct ppg_material {
    int32_t type;         /* PPG_BSDF_* */
    float reflectance[3]; /* linear RGB (SPECTRUM_SAMPLES=3 build of the reference): diffuse / roughdiffuse `reflectance`; plastic / phong
                             `diffuseReflectance`; conductors and dielectric `specularReflectance`; difftrans `transmittance` */
    float specular[3];    /* plastic / phong `specularReflectance`; dielectric / thindielectric `specularTransmittance` */
    float alpha;          /* roughconductor / roughdielectric: roughness `alpha` (clamped to >= 1e-4 like microfacet.h:135);
                             roughdiffuse: `alpha` (default 0.2; NOT clamped, 0 is legal); phong: `exponent` (default 30).  The last two
                             must be finite and >= 0 */
    float eta[3];         /* conductors: eta per channel (already divided by extEta, roughconductor.cpp:185-186);
                             plastic / (rough / thin) dielectric: eta[0] = intIOR / extIOR */
    float k[3];           /* conductors: k per channel */
    int32_t flags;        /* PPG_MAT_* */
    int32_t rtrans;       /* roughplastic: index of this material's slice in ppg_scene.rtrans; otherwise 0 */
    float opacity[3];     /* PPG_MAT_MASK: opacity (mask.cpp, default 0.5) */
    uint32_t texture;     /* bits 0..15: 1 + index (ppg_scene.textures) of the bitmap on `reflectance` — `reflectance` of diffuse,
                             `diffuseReflectance` of plastic / roughplastic, `specularReflectance` of conductor / roughconductor / dielectric /
                             thindielectric / roughdielectric — in which case reflectance[] holds the texture's average
                             (Texture::getAverage, used by the plug-ins' configure() for the component sampling weights, plastic.cpp:191-204);
                             bits 16..31: 1 + index of the displacement texture of a `bumpmap` adapter around this BSDF (bumpmap.cpp:135-219:
                             shading frame perturbed by the texture's gradient) or, with PPG_MAT_NORMALMAP, of the normal map of a `normalmap`
                             adapter (normalmap.cpp:108-124: shading frame around the texel's normal); 0 = none */
} ppg_material;           /* 80 bytes; bitmaps on specular / alpha / opacity: ppg_set_material_textures */
/* roughdiffuse, difftrans and phong (HIP library only).  PPG_MAT_TWOSIDED (not on difftrans), PPG_MAT_MASK and both halves of `texture` apply
   as they do to diffuse: bumpmap(mask(twosided(x))).  ppg_set_scene answers PPG_ERR_INVALID, names the material and leaves the context
   usable for: PPG_MAT_TWOSIDED on difftrans (twosided.cpp:84-88 refuses transmissive BSDFs); a phong whose reflectance and specular both
   have luminance 0 (specularSamplingWeight = 0 / 0); a negative or non-finite alpha / exponent; PPG_MAT_FAST_APPROX on another type; any slot
   of ppg_set_material_textures but `opacity`; a general ppg_set_microfacet entry; a coat (ppg_set_coatings); their use as a child of a blend
   or as the blended record (ppg_set_blends); and, as for every type, a bitmap on a material of a sphere, disk or cylinder.
   PPG_MAT_NORMALMAP (HIP library only) follows the rules of a bump-mapped record — not on a sphere, disk or cylinder, not on the child of a
   blend, normalmap(mask(twosided(x))) with x a leaf, a coat or a blend — and is refused, in the same way, when bits 16..31 of `texture` are 0.
   A texel that decodes to the zero vector gives Mitsuba's NaN frame; keep such texels out of a normal map.
   PPG_BSDF_NULL (HIP library only) is refused, in the same way, with PPG_MAT_TWOSIDED (twosided.cpp:84-88), PPG_MAT_MASK or any other flag, any
   `texture` word or slot of ppg_set_material_textures, a general ppg_set_microfacet entry, a coat, as a child of a blend or as the blended
   record, and on a sphere, disk or cylinder.  An emitter id on its triangles works as on any material. */

typedef struct ppg_emitter {
    float radiance[3]; /* area light, mitsuba/src/emitters/area.cpp:104-109 */
    float _pad;
} ppg_emitter;

typedef struct ppg_sphere {
    /* An analytic sphere (shapes/sphere.cpp:106-372): double-precision quadratic for the ray test (:164-189), intersection record and
       (theta, phi) tangent frame of :213-263, Shirley et al. cone sampling / uniform area sampling for next-event estimation
       (:291-378).  Spheres are primitives number n_triangles, n_triangles + 1, .. for the closest-hit tie rule. */
    float center[3];
    float radius;         /* > 0 (sphere.cpp:129-130); the scale of `toWorld` is folded in (:113-121) */
    float to_world[9];    /* row-major rotation left of `toWorld` once its scale is removed (m_objectToWorld's linear part, :116-120);
                             identity for an untransformed sphere.  The inverse is taken as the transpose. */
    uint32_t material;    /* index into materials */
    int32_t emitter;      /* index into emitters, -1 = none; an emitter id carried by a sphere must not be used by any other shape */
    int32_t flip_normals; /* sphere.cpp:124, 256-257, 351-352 */
} ppg_sphere;             /* 64 bytes */

typedef struct ppg_envmap {
    /* Image-based environment emitter (emitters/envmap.cpp): a latitude-longitude radiance map, bilinearly interpolated
       (mipmap.h:575-596, repeat in u / clamp in v), importance-sampled by luminance x sin(theta) with the tent-filtered pixel
       sampling of envmap.cpp:557-595 and its pdf (:598-633); the bounding sphere / emitter numbering of the constant emitter.
       Deviation: a camera ray that leaves the scene is looked up bilinearly at level 0 as well (the reference filters it with
       EWA over the ray differentials, envmap.cpp:389-404) — this only smooths the directly visible background. */
    uint32_t width, height;   /* <= 65535 */
    const float *rgb;         /* [height * width * 3] linear RGB, row 0 = +y (theta = 0), column 0 = -z turning towards +x */
    float scale;              /* envmap.cpp:189 */
    float to_world[9];        /* row-major rotation of the emitter's toWorld (inverse taken as transpose); identity if none */
} ppg_envmap;

typedef struct ppg_camera {
    /* row-major 4x4, exactly the matrices of mitsuba/src/sensors/perspective.cpp:150-164 (m_sampleToCamera)
       and the sensor's world transform; rays follow perspective.cpp:271-298 */
    float sample_to_camera[16];
    float camera_to_world[16];
    float near_clip, far_clip;
    int32_t width, height; /* film / crop size in pixels */
} ppg_camera;

typedef struct ppg_scene {
    uint32_t n_vertices;
    const float *positions;       /* [n_vertices*3] */
    const float *normals;         /* [n_vertices*3] or NULL → face normals (skdtree.h:388-401) */
    uint32_t n_triangles;
    const uint32_t *indices;      /* [n_triangles*3] */
    const uint32_t *tri_material; /* [n_triangles] index into materials */
    const int32_t *tri_emitter;   /* [n_triangles] index into emitters, -1 = not an emitter */
    uint32_t n_materials;
    const ppg_material *materials;
    uint32_t n_emitters;
    const ppg_emitter *emitters;
    ppg_camera camera;
    const float *environment;     /* NULL, or float[3]: radiance of a constant environment emitter (emitters/constant.cpp) — what rays
                                     that leave the scene see (GP:1902-1914, 2236-2243) and one more emitter for luminaire sampling */
    /* Rough-transmittance slices for PPG_BSDF_ROUGHPLASTIC (0 / 0 / NULL without such materials).  One slice per (distribution, alpha,
       eta) = what RoughPlastic::configure() (roughplastic.cpp:285-305) leaves in its two RoughTransmittance objects:
         [0 .. rtrans_samples)  m_externalRoughTransmittance after setEta(eta), setAlpha(alpha) (rtrans.h:299-400): transmittance over
                                the warped incident cosine |cos|^(1/4) in [0, 1], read by eval() through evalCubicInterp1D;
         [rtrans_samples]       m_internalRoughTransmittance->evalDiffuse(alpha) after setEta(1/eta) (the diffuse transmittance from
                                inside: 1 - Fdr, roughplastic.cpp:372). */
    uint32_t n_rtrans;
    uint32_t rtrans_samples;      /* thetaSamples of the data file (100 in Mitsuba's tables), >= 2 */
    const float *rtrans;          /* [n_rtrans * (rtrans_samples + 1)] */
    uint32_t n_spheres;
    const ppg_sphere *spheres;    /* [n_spheres] or NULL */
    const ppg_envmap *envmap;     /* NULL, or the image-based environment emitter (not together with `environment`) */
    const float *texcoords;       /* NULL, or [n_vertices * 2] per-vertex texture coordinates (TriMesh::m_texcoords; its.uv is their barycentric
                                     interpolation, skdtree.h:403-410 — without them its.uv = the barycentrics (b1, b2)).  A triangle whose three
                                     vertices all carry NaN has no texture coordinates (meshes with and without `vt` share the vertex array).
                                     Triangles WITH coordinates whose BSDF uses a texture also get the reference's UV tangents as dpdu / dpdv
                                     (TriMesh::computeUVTangents, trimesh.cpp:683-735; skdtree.h:374-381) */
    uint32_t n_textures;
    const ppg_texture *textures;  /* [n_textures] or NULL */
} ppg_scene;

/* ------------------------------------------------------------------------------------------------
 * Statistics returned by the stepwise calls (the numbers the reference logs).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_pass_stats {   /* GP:1321-1326 "… seconds, Total passes, Var, TTUV, STUV" */
    double seconds;
    int32_t passes_rendered_total;
    int32_t passes_rendered_local;
    float variance;
    uint64_t samples;             /* pixels × spp rendered by this call (this shard) */
    uint64_t rays;                /* "Normal rays traced" (skdtree.cpp:46,123) */
    uint64_t path_length_sum;     /* Σ rRec.depth, avgPathLength GP:2147-2148 */
    uint64_t vertices_committed;  /* records that reached DTreeWrapper::record */
} ppg_pass_stats;

typedef struct ppg_tree_stats {   /* GP:1176-1186 "Distribution statistics" */
    int32_t min_depth, max_depth;  float avg_depth;
    float min_mean_radiance, avg_mean_radiance, max_mean_radiance;
    uint64_t min_nodes, max_nodes; float avg_nodes;
    float min_stat_weight, avg_stat_weight, max_stat_weight;
    uint32_t n_leaves;            /* S-tree leaves (nPoints, GP:1135) */
    uint32_t n_stree_nodes;
    uint64_t n_dtree_nodes;       /* Σ numNodes over the sampling D-trees */
} ppg_tree_stats;

/* ------------------------------------------------------------------------------------------------
 * Life cycle.
 * ---------------------------------------------------------------------------------------------- */
/* Replaces CreateInstance(props) → new GuidedPathTracer(props) (cobject.h:99-107, GP:1014, 2421-2422). */
int ppg_create(const ppg_config *cfg, ppg_ctx **out);
void ppg_destroy(ppg_ctx *ctx);
const char *ppg_last_error(const ppg_ctx *ctx); /* ctx may be NULL: error of the last failed ppg_create */
const char *ppg_description(void);              /* GetDescription(), cobject.h:107: "Guided path tracer" */

/* Replaces Scene::preprocess/initialize as far as this path needs it (scene.cpp:322-384): copies the
   triangles, builds the BVH that stands in for the SAH kd-tree (skdtree.cpp:112-142), uploads.
   The scene is validated and built on the host before the context is touched: PPG_ERR_INVALID leaves the previous scene set and
   renderable exactly as before, PPG_ERR_DEVICE (a failed upload) leaves no scene set. */
int ppg_set_scene(ppg_ctx *ctx, const ppg_scene *scene);

/* Multi-GPU image sharding (no reference counterpart; BlockedRenderProcess hands 32×32 blocks to
   worker threads, renderproc.cpp:69-87).  Tile t (row-major, tile_size² pixels) is rendered by
   rank t % world.  Default: rank 0 of 1. */
int ppg_set_shard(ppg_ctx *ctx, int32_t rank, int32_t world, int32_t tile_size);

/* ------------------------------------------------------------------------------------------------
 * Film reconstruction filter: the <rfilter> of the scene's hdrfilm (mitsuba/src/rfilters/; Mitsuba's default is gaussian,
 * mitsuba/src/librender/film.cpp:89-95).  Parameters, defaults and radius as in Mitsuba:
 *   box         radius (0.5) + 1e-5           tent        radius 1
 *   gaussian    stddev (0.5), radius 4 stddev  mitchell    B, C (1/3, 1/3), radius 2
 *   catmullrom  radius 2                      lanczos     lobes (3), radius lobes
 * A sample at samplePos is splatted like ImageBlock::put (imageblock.h:147-190): pos = samplePos - 0.5, the pixels x in
 * [ceil(pos.x - r), floor(pos.x + r)] (likewise y) clipped to the film, weight = evalDiscretized(x - pos.x) * evalDiscretized(y - pos.y)
 * from the 32-entry table of ReconstructionFilter::configure (rfilter.cpp:37-55); image += w L, squared image += w L², weights += w, for
 * the film and for the per-pass image of the variance estimate alike (renderBlock puts every sample into both blocks, GP:1604-1640).
 *   - The default box (radius 0.5) keeps the own-pixel, unit-weight film.  Deviation: Mitsuba's box radius is 0.5 + 1e-5, so a sample
 *     within 1e-5 of a pixel edge also reaches the neighbouring pixel; this build ignores that sliver.
 *   - Every other filter (a box of another radius included) splats into at most (2B + 1)² pixels, B = ceil(r - 0.5) <= 3 (7 x 7);
 *     a larger border is PPG_ERR_INVALID.  A pixel the reference would reach outside that window (only when r + 0.5 is an integer and
 *     the sample lies exactly on a pixel edge: its weight is the table's 0 entry) is left out.
 *   - No float atomics; the sums have ONE association, independent of batch size, launch schedule and thread count: per source pixel,
 *     its samples in sample order into a footprint slot per target pixel (tap); per target pixel, its taps in the order dy = -B .. B and,
 *     within each dy, dx = -B .. B, starting from zero; then, in a final iteration ("groups of passes" below), the groups in group order.
 *   - Sharded by tiles (ppg_set_shard, world > 1) a rank holds the footprint slots of ITS source pixels only; the ranks exchange the slots
 *     that cross a tile border between two of them through the footprint hook ("Footprint hook" below), each rank resolves its own
 *     target pixels in the order above, and the film is one GPU's, bit for bit.  Without a hook on the context a filter other than the
 *     default box together with world > 1 stays PPG_ERR_INVALID, whichever of ppg_set_rfilter / ppg_set_shard comes second.
 * ---------------------------------------------------------------------------------------------- */
enum { PPG_RFILTER_BOX = 0, PPG_RFILTER_TENT, PPG_RFILTER_GAUSSIAN, PPG_RFILTER_MITCHELL, PPG_RFILTER_CATMULLROM, PPG_RFILTER_LANCZOS };
typedef struct ppg_rfilter {
    int32_t type;   /* PPG_RFILTER_* */
    float radius;   /* box */
    float stddev;   /* gaussian */
    float B, C;     /* mitchell */
    int32_t lobes;  /* lanczos */
} ppg_rfilter;
void ppg_rfilter_default(ppg_rfilter *f);                 /* box, radius 0.5 (and the other types' defaults in their fields) */
int ppg_set_rfilter(ppg_ctx *ctx, const ppg_rfilter *f); /* before ppg_begin_render; NULL = default */

/* ------------------------------------------------------------------------------------------------
 * Thin-lens camera (mitsuba/src/sensors/thinlens.cpp: ThinLens::sampleRayDifferential, :321-356).  The scene's ppg_camera stays what it
 * is (sample_to_camera, camera_to_world, clip distances: the perspective camera's own); the lens adds an aperture disk of radius
 * aperture_radius (world units) and a focal plane at focus_distance along the camera's z axis.  Per sample:
 *   dims 0, 1  pixel position, as for the pinhole;  dims 2, 3  aperture sample (renderBlock draws it right after the pixel sample when the
 *   sensor needs one, GP:1613-1630); the path continues from dim 4 (a pinhole's path still starts at dim 2).
 *   (tx, ty) = squareToUniformDiskConcentric(dims 2, 3) * aperture_radius;  apertureP = (tx, ty, 0)
 *   nearP = sample_to_camera(pixel / resolution);  focusP = nearP * (focus_distance / nearP.z);  d = normalize(focusP - apertureP)
 *   mint = near_clip / d.z, maxt = far_clip / d.z;  origin = camera_to_world.transformAffine(apertureP), direction = camera_to_world(d)
 * The scene's box (the SD-tree's domain, the environment's bounding sphere) takes in the aperture disk instead of the pinhole position
 * (Scene::initializeBidirectional, thinlens.cpp:516-520).
 * NULL = pinhole (the default).  Call before ppg_begin_render.  The lens belongs to the context, not to the scene: ppg_set_scene keeps it
 * (like the reconstruction filter).  A radius or distance that is not finite and above 0 is PPG_ERR_INVALID (the loaders turn Mitsuba's
 * apertureRadius 0 into Epsilon = 1e-4 first, as ThinLens does).  Sharded renders need nothing more: the lens acts per sample.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_lens {
    float aperture_radius, focus_distance;
} ppg_lens;
int ppg_set_lens(ppg_ctx *ctx, const ppg_lens *lens);

/* ------------------------------------------------------------------------------------------------
 * Delta emitters: Mitsuba's `point`, `spot` and `directional` plug-ins (mitsuba/src/emitters/point.cpp, spot.cpp, directional.cpp).  They
 * are sampled by next-event estimation only (Emitter::sampleDirect); nothing can hit them, so with nee = never — and in every iteration
 * in which kickstart has switched NEE off — they contribute nothing, as in the reference.  Per direct-light sample at `ref`:
 *   point        d = position - ref, dist = |d|, d *= 1 / dist;  value = intensity * (1 / dist)^2
 *   spot         the same, times falloffCurve(to_local * (-d)): with cosTheta = the z component, 0 for cosTheta <= cos(cutoff_angle),
 *                1 for cosTheta >= cos(beam_width), else (cutoff_angle - acos(cosTheta)) / (cutoff_angle - beam_width)   (spot.cpp:89-125)
 *   directional  distance = dot(ref - diskCenter, direction), diskCenter = centre - direction * radius of the bounding sphere of the
 *                GEOMETRY's box (the kd-tree's, not the box enlarged by sensor and emitters) with its radius * 1.1; a negative distance
 *                gives zero; else d = -direction, n = direction, dist = distance, value = irradiance   (directional.cpp:56-101, 159-180)
 *   all three    n = 0 (directional: the direction), pdf = 1, discrete measure: the integrator does not evaluate the BSDF / D-tree
 *                densities, miWeight(pdf, 0) = 1 (GP:1987-1994), and no area-emitter facing test applies.  The shadow segment runs to
 *                the light's point undiminished (the emitter is not on a surface, scene.cpp:625).
 * Emitter numbering (the uniform emitter choice of Scene::configure, scene.cpp:375-380): the scene's area emitters 0 .. n_emitters - 1,
 * then the delta emitters in the order given here, then the environment emitter.  With no delta emitters every index and table is what
 * it is without this call.
 * Scene box (Scene::initializeBidirectional, scene.cpp:400-413): the box — the SD-tree's domain, the basis of the environment emitter's
 * bounding sphere — takes in the positions of point and spot emitters; a directional emitter adds nothing.
 * Call before ppg_set_scene, which consumes the list; the context keeps the list until it is replaced (n = 0 clears it), and a later
 * ppg_set_scene uses it again.  Between ppg_begin_render and ppg_end_render the call is PPG_ERR_STATE.  PPG_ERR_INVALID: an unknown type, a
 * value that is not finite, a negative intensity, angles outside 0 < beam_width <= cutoff_angle < pi/2 (spot), a zero direction
 * (directional).  The scene then renders with the FULL kernel variants, like one with an environment emitter.
 * The CPU oracle does not know these emitters: nothing pins them against it.  They are pinned by a restatement of every sample of a
 * direct-light-only scene and statistically against a tiny spherical area emitter, which the oracle does pin.
 * ---------------------------------------------------------------------------------------------- */
#define PPG_EMITTER_POINT 0
#define PPG_EMITTER_SPOT 1
#define PPG_EMITTER_DIRECTIONAL 2
typedef struct ppg_delta_emitter {
    int32_t type;          /* PPG_EMITTER_* */
    float intensity[3];    /* RGB intensity (point, spot: power per unit solid angle) or irradiance (directional) */
    float position[3];     /* point, spot: world position */
    float to_local[9];     /* spot: row-major 3x3 of toWorld's inverse — takes world directions into the light's frame, whose +z is the axis */
    float direction[3];    /* directional: the direction the light travels in (toWorld applied to (0, 0, 1)): a unit vector, used as given */
    float cutoff_angle, beam_width; /* spot: radians */
} ppg_delta_emitter;
int ppg_set_delta_emitters(ppg_ctx *ctx, const ppg_delta_emitter *emitters, uint32_t n);

/* ------------------------------------------------------------------------------------------------
 * Analytic disks and cylinders (shapes/disk.cpp, shapes/cylinder.cpp), as surfaces and as area emitters.  ppg_scene and ppg_sphere keep
 * their layout: this is a side list like the delta emitters'.  The shapes are primitives number n_triangles + n_spheres + k for the
 * closest-hit tie rule (a shape beats an earlier primitive only with a strictly smaller t), tested one after the other behind the BVH.
 *   disk      the unit disk z = 0, x^2 + y^2 <= 1 of object space under `to_world` (any rotation, translation and UNIFORM scale).  The
 *             ray goes to object space through the float inverse; hit = -o.z / d.z, then x^2 + y^2 <= 1 (disk.cpp:139-162).  Normal =
 *             normalize(to_world applied to Normal(0, 0, 1)), negated by flip_normals — which is all that the constructor's prepended
 *             scale(1, 1, -1) does; tangent = the radial direction (the x axis at r = 0).  Area sampling by
 *             squareToUniformDiskConcentric, pdf 1 / (pi |column 0|^2) (:101-115, 247-255).  `radius` and `length` are ignored.
 *   cylinder  the open tube x^2 + y^2 = radius^2, 0 <= z <= length of object space under `to_world`, which is m_objectToWorld AFTER the
 *             constructor has removed the scale (cylinder.cpp:99-103): a rotation and a translation.  Double-precision quadratic in
 *             x, y, then the near / far rules with the z tests (:128-165; the any-hit form :167-199 differs in its maxt test, and so does
 *             the shadow trace here).  No end caps.  Record of :201-230: dpdu = (-y, x, 0) 2 pi, n = cross(normalize(dpdu),
 *             normalize(dpdv)), p re-projected radially, then flip_normals.  Area sampling p = (r cos 2 pi v, r sin 2 pi v, u length),
 *             pdf 1 / (2 pi r length) (:232-246).
 * As emitters both go through Shape::sampleDirect (shape.cpp:97-115): area density to solid angle, dist^2 / |dot(d, n)|, and the same
 * density on the hit side.  One deviation from the reference: its disk never sets its.geoFrame, so strictNormals reads a stale frame
 * there; here the geometric normal of a disk hit is its shading normal.
 * Scene box: grows by Disk::getAABB (the four points (+-1, 0, 0), (0, +-1, 0) transformed, :117-130) and Cylinder::getAABB (:252-273).
 * Call before ppg_set_scene, which validates and consumes the list; the context keeps it until it is replaced (n = 0 clears it).
 * Between ppg_begin_render and ppg_end_render the call is PPG_ERR_STATE.  A scene may consist of such shapes only.  ppg_set_scene returns
 * PPG_ERR_INVALID, with the shape's index in ppg_last_error, for: an unknown type; a value that is not finite; a disk whose to_world
 * shears (|dot(normalize(col0), normalize(col1))| > 1e-3), scales non-uniformly (| |col0| / |col1| - 1 | > 1e-3) or is singular; a
 * cylinder with radius <= 0, length <= 0 or a linear part that is not a rotation (the same 1e-3 tests, and column lengths within 1e-3
 * of 1); a material index out of range; an emitter id shared with any other shape; a material with a texture word or a
 * ppg_set_material_textures slot.  Such scenes render with the FULL kernel variants on the BVH path.
 * The CPU oracle does not know these shapes; they are pinned ray by ray and sample by sample through include/ppg_testhooks.h.
 * ---------------------------------------------------------------------------------------------- */
#define PPG_SHAPE_DISK 0
#define PPG_SHAPE_CYLINDER 1
typedef struct ppg_shape {
    int32_t type;          /* PPG_SHAPE_*                                                        offset  0 */
    float to_world[12];    /* row-major 3x4 object-to-world                                              4 */
    float radius, length;  /* cylinder: m_radius, m_length; disk: ignored                           52, 56 */
    uint32_t material;     /* index into materials                                                      60 */
    int32_t emitter;       /* index into emitters, -1 = none; not shared with any other shape           64 */
    int32_t flip_normals;  /*                                                                           68 */
    uint32_t _reserved[2]; /* 0                                                                         72 */
} ppg_shape;               /* 80 bytes */
int ppg_set_shapes(ppg_ctx *ctx, const ppg_shape *shapes, uint32_t n);

/* ------------------------------------------------------------------------------------------------
 * Bitmaps on the other material parameters (ppg_material keeps its 80 bytes: this is a side list, one entry per material in
 * ppg_scene.materials' order).  Each slot is 1 + an index into ppg_scene.textures, 0 = none, and names the ppg_material field it replaces
 * at every intersection by the texture's value at its.uv (wherever the plug-ins call m_...->eval(bRec.its)):
 *   specular  `specularReflectance` of plastic / roughplastic; `specularTransmittance` of dielectric / thindielectric / roughdielectric
 *   alpha     `alpha` of roughconductor / roughdielectric: eval(its).average() = (r + g + b) / 3, then clamped to >= 1e-4 like the constant
 *   opacity   `opacity` of a PPG_MAT_MASK material (mask.cpp:115): looked up at the shading hit AND at every surface a shadow segment
 *             (Scene::evalTransmittance) or the search for an emitter behind null surfaces (GP:2184-2245) passes through
 * The lookup is ppg_texture's (same filter flag, wrap modes, uv scale / offset; uv = the barycentrics on a mesh without texture coordinates).
 * The record's field holds the texture's average (Texture::getAverage), as reflectance[] does under ppg_material.texture: the plug-ins'
 * configure() derives the component sampling weights of plastic / roughplastic from the averages, not from the looked-up values
 * (plastic.cpp:199-200, roughplastic.cpp:275-276).  A material with a slot has the shading frame of a textured one (the UV tangents).
 * Call before ppg_set_scene, which validates and consumes the list; the context keeps the list until it is replaced (n_materials = 0
 * clears it), and a later ppg_set_scene uses it again.  Between ppg_begin_render and ppg_end_render the call is PPG_ERR_STATE.
 * ppg_set_scene then returns PPG_ERR_INVALID, naming material and slot in ppg_last_error, for: a list whose length is neither 0 nor the
 * scene's n_materials; an index beyond n_textures; a slot on a BSDF type that does not read the field (above); opacity without
 * PPG_MAT_MASK; alpha on roughplastic (its rough-transmittance slice is tabulated for ONE alpha, roughplastic.cpp:295-298); _reserved != 0;
 * a material with a slot on an analytic sphere.  Any non-zero slot selects the FULL kernel variants, as ppg_material.texture does.
 * The CPU oracle does not know these slots: nothing pins them against it.  They are pinned by reduction — a constant texture renders bit
 * for bit what the constant does, which the oracle pins; a shared texture what per-material 1x1 textures do — and by closed forms for a
 * directly seen specular colour and for cut-outs seen directly and as shadows.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_material_textures {
    uint32_t specular, alpha, opacity, _reserved;
} ppg_material_textures;
int ppg_set_material_textures(ppg_ctx *ctx, const ppg_material_textures *slots, uint32_t n_materials);

/* ------------------------------------------------------------------------------------------------
 * The rest of Mitsuba's MicrofacetDistribution (microfacet.h) for roughconductor / roughdielectric / roughplastic: alphaU / alphaV,
 * distribution = phong (Phong, anisotropic: Ashikhmin-Shirley) and sampleVisible = false.  Another side list, one entry per material in
 * ppg_scene.materials' order, with the ordering rules of ppg_set_material_textures: call before ppg_set_scene, which validates and
 * consumes it; the context keeps it until it is replaced (NULL or n_materials = 0 clears it, and a cleared list renders exactly as a fresh
 * context does); PPG_ERR_STATE between ppg_begin_render and ppg_end_render.
 * An entry with general = 0 leaves the material on the isotropic path of ppg_material (its other fields are ignored).  With general != 0
 *   alphaU        is ppg_material.alpha (and the alpha slot of ppg_material_textures), alphaV is alpha_v (alpha_v_texture: 1 + index into
 *                 ppg_scene.textures, 0 = none; eval(its).average(), as alpha); both clamped to >= 1e-4 (microfacet.h:135-136)
 *   distribution  0: ggx, or beckmann with PPG_MAT_BECKMANN; 1: phong, which implies sample_all (microfacet.h:141-142)
 *   sample_all    sampleVisible = false: sampleAll / pdfAll instead of the visible normals, with the plug-ins' other weights
 *                 (roughconductor.cpp:316-320, 403-409) and roughdielectric's scaled sampling roughness (roughdielectric.cpp:406-411)
 * An anisotropic material (alpha_v != alpha, or either from a bitmap) has the shading frame of a textured one, the UV tangents
 * (trimesh.cpp:380); analytic spheres, disks and cylinders span theirs from their own dpdu.
 * ppg_set_scene returns PPG_ERR_INVALID for: a list whose length is neither 0 nor n_materials; general on another BSDF type; roughplastic
 * with alpha_v != alpha (roughplastic.cpp:221) or with an alpha_v_texture; a distribution other than 0 / 1; a non-zero reserved word; a
 * texture index out of range; a triangle with an anisotropic material on a mesh without texture coordinates (trimesh.cpp:686-691).
 * A scene with a general entry runs the "extended" kernels (csrc: PPG_MFD), whatever else it holds; the CPU oracle does not know these
 * entries (they are pinned by reduction to the isotropic path and against a float64 restatement).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_microfacet {
    float alpha_v;            /* alphaV; alphaU stays ppg_material.alpha (and its alpha bitmap slot) */
    int32_t distribution;     /* 0 = as ppg_material.flags says (ggx / PPG_MAT_BECKMANN), 1 = phong */
    int32_t sample_all;       /* sampleVisible = false */
    uint32_t alpha_v_texture; /* 1 + index into ppg_scene.textures, 0 = none */
    uint32_t general;         /* 0 = this material keeps the isotropic path and the other fields are ignored */
    uint32_t _reserved[3];    /* must be 0 */
} ppg_microfacet;             /* 32 bytes */
int ppg_set_microfacet(ppg_ctx *ctx, const ppg_microfacet *m, uint32_t n_materials);

/* ------------------------------------------------------------------------------------------------
 * Mitsuba's `coating` (coating.cpp, SmoothCoating) and `roughcoating` (roughcoating.cpp, RoughCoating) adapters: a dielectric layer
 * over the material's BSDF, inside its two-sided / mask / bump-map adapters: bumpmap( mask( twosided( coat( leaf )))).  One more side
 * list, one entry per material in ppg_scene.materials' order, with the ordering rules of ppg_set_material_textures: call before
 * ppg_set_scene, which validates and consumes it; the context keeps it until it is replaced (NULL or n_materials = 0 clears it);
 * PPG_ERR_STATE between ppg_begin_render and ppg_end_render.  A list without an entry of kind != 0 renders exactly as no list does.
 *   kind          0: none (the other fields are ignored), 1: coating, 2: roughcoating
 *   eta           intIOR / extIOR;  thickness, sigma_a: the layer's absorption exp(-sigma_a * thickness * (1/|cos i'| + 1/|cos o'|))
 *   specular      specularReflectance of the layer's own (delta / glossy) reflection, the BSDF's last component
 *   kind 2:       alpha (clamped to >= 1e-4), distribution (0 beckmann, 1 ggx, 2 phong, which implies sample_all), sample_all
 *                 (sampleVisible = false) and rtrans: the layer's rough-transmittance slice, a row of ppg_scene.rtrans — the reduction
 *                 roughplastic uses, for (distribution, alpha, eta)
 * specularSamplingWeight = 1 / (avg(exp(-2 * thickness * sigma_a)) + 1) is derived inside ppg_set_scene with the library's own exp.
 * Nested BSDFs: coating takes diffuse, mirror / conductor, roughconductor, plastic and roughplastic; roughcoating those without a delta
 * component — diffuse, roughconductor, roughplastic.  ppg_set_scene returns PPG_ERR_INVALID, and ppg_last_error names the material, for:
 * a list whose length is neither 0 nor n_materials; another kind; a coat on dielectric, thindielectric or roughdielectric; a
 * roughcoating over mirror, conductor or plastic; eta <= 0 or == 1; a value that is not finite; negative thickness or sigma_a; a
 * distribution other than 0..2; rtrans out of range; a non-zero reserved word.
 * A scene with a coat runs the "coat" kernels (csrc: PPG_COAT), whatever else it holds; the CPU oracle does not know these entries
 * (they are pinned against a float64 restatement).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_coating {
    int32_t kind;          /* 0 = none, 1 = coating, 2 = roughcoating */
    float eta;             /* intIOR / extIOR */
    float thickness;
    float sigma_a[3];
    float specular[3];     /* specularReflectance */
    float alpha;           /* kind 2 */
    int32_t distribution;  /* kind 2: 0 = beckmann, 1 = ggx, 2 = phong */
    int32_t sample_all;    /* kind 2: sampleVisible = false */
    int32_t rtrans;        /* kind 2: row of ppg_scene.rtrans */
    uint32_t _reserved[3]; /* must be 0 */
} ppg_coating;             /* 64 bytes */
int ppg_set_coatings(ppg_ctx *ctx, const ppg_coating *c, uint32_t n_materials);

/* ------------------------------------------------------------------------------------------------
 * Mitsuba's `blendbsdf` (blendbsdf.cpp) and `mixturebsdf` (mixturebsdf.cpp) combinators: a material that interpolates, or linearly
 * combines, other entries of ppg_scene.materials.  One more side list, one entry per material, with the ordering rules of
 * ppg_set_coatings: call before ppg_set_scene, which validates and consumes it; the context keeps it until it is replaced (NULL or
 * n_materials = 0 clears it); PPG_ERR_STATE between ppg_begin_render and ppg_end_render.  A list whose entries are all of kind 0 renders
 * exactly as no list does.
 *   kind     0: none (the other fields are ignored), 1: blendbsdf, 2: mixturebsdf
 *   n        the number of children: 2 for blendbsdf, 1 .. PPG_BLEND_MAX for mixturebsdf
 *   child    indices into ppg_scene.materials.  A child is an ordinary material — triangles may use it directly as well —: diffuse,
 *            mirror / conductor, roughconductor, plastic or roughplastic, with its reflectance bitmap, its specular / alpha slots
 *            (ppg_set_material_textures) and its entry of ppg_set_microfacet; not blended, coated, masked, two-sided or bump-mapped itself
 *   weight   kind 1: weight[0] = `weight` (clamped to [0, 1]; the children get 1 - w and w); kind 2: the `weights`, >= 0 with a sum > 0
 *   weight_texture  kind 1: 1 + index into ppg_scene.textures of a bitmap `weight` (its average at the hit's uv, clamped), 0 = none
 *   ensure_energy_conservation  kind 2: weights whose sum exceeds 1 are multiplied by 1 / sum (mixturebsdf.cpp:130-141)
 * The rescaled weights and the normalised DiscreteDistribution (pmf.h: running float sum, then normalize()) are derived inside
 * ppg_set_scene with the library's own float arithmetic.
 * The blended material's own ppg_material record supplies the adapters around the blend, bumpmap( mask( twosided( blend( .. )))): its
 * flags (PPG_MAT_TWOSIDED, PPG_MAT_MASK), opacity, the opacity slot and the bump-map half of `texture` apply; its type must be
 * PPG_BSDF_DIFFUSE and its BSDF fields are otherwise ignored.
 * ppg_set_scene returns PPG_ERR_INVALID, and ppg_last_error names the material, for: a list whose length is neither 0 nor n_materials;
 * another kind; n or a child index out of range; a child that is itself blended, coated, masked, two-sided or bump-mapped; a dielectric,
 * thindielectric or roughdielectric child; a coat on the blended material; a reflectance bitmap, a parameter slot (other than opacity
 * with PPG_MAT_MASK) or a microfacet entry on the blended record; a type other than PPG_BSDF_DIFFUSE there; a weight that is negative or
 * not finite; a mixture whose weights sum to 0; a texture index out of range; a non-zero reserved word; a blend on an analytic sphere or
 * shape when it or a child reads a bitmap; an anisotropic child on a mesh without texture coordinates.
 * A scene with a blended material runs the "blend" kernels (csrc: PPG_BLEND), whatever else it holds; the CPU oracle does not know these
 * entries (they are pinned against a float64 restatement).
 * ---------------------------------------------------------------------------------------------- */
#define PPG_BLEND_MAX 4
typedef struct ppg_blend {
    int32_t kind;                        /* 0 = none, 1 = blendbsdf, 2 = mixturebsdf */
    uint32_t n;                          /* children */
    uint32_t child[PPG_BLEND_MAX];       /* indices into ppg_scene.materials */
    float weight[PPG_BLEND_MAX];
    uint32_t weight_texture;             /* kind 1: 1 + texture index, 0 = none */
    int32_t ensure_energy_conservation;  /* kind 2 */
    uint32_t _reserved[4];               /* must be 0 */
} ppg_blend;                             /* 64 bytes */
int ppg_set_blends(ppg_ctx *ctx, const ppg_blend *b, uint32_t n_materials);

/* ------------------------------------------------------------------------------------------------
 * Homogeneous participating media (medium/homogeneous.cpp) with the `isotropic` and `hg` phase functions (phase/isotropic.cpp, hg.cpp):
 * the medium branch of GuidedPathTracer::Li (GP:1803-1893), its failure factor (GP:1899-1911), the medium carried through surface
 * bounces (GP:2041-2042), shadow segments (Scene::evalTransmittance, scene.cpp:619-679) and the search for an emitter behind null
 * surfaces (GP:2184-2245).  The SD-tree guides at surfaces only: a medium event makes no vertex and looks up no D-tree, and the radiance
 * found behind it is recorded into the surface vertices in front of it.
 * One more side list, with the ordering rules of the others: call before ppg_set_scene, which validates and consumes it; the context
 * keeps it until it is replaced (NULL or n_media = 0 clears it, and a cleared list renders exactly as a fresh context does);
 * PPG_ERR_STATE between ppg_begin_render and ppg_end_render.
 *   media          the media.  sigma_a, sigma_s are Mitsuba's sigmaA, sigmaS AFTER `scale` (sigmaT + albedo: sigma_s = sigmaT * albedo,
 *                  sigma_a = sigmaT - sigma_s, medium.cpp); sigmaT = sigma_a + sigma_s is derived inside ppg_set_scene
 *   strategy       PPG_MEDIUM_BALANCE (a second random number picks the channel whose sigmaT is the sampling density), _SINGLE
 *                  (sampling density = sigmaT[channel]; channel < 0: the channel with the smallest sigmaT) or _MANUAL (sampling_density)
 *   sampling_weight  mediumSamplingWeight in [0, 1], or -1: derive it — the highest albedo over the channels with sigmaT != 0, raised to
 *                  at least 0.5 when it is positive (homogeneous.cpp:168-184); a pure absorber gets 0 and never scatters
 *   phase, g       PPG_PHASE_ISOTROPIC, or PPG_PHASE_HG with g in (-1, 1)
 * A binding word names the media on the two sides of a primitive: low 16 bits = 1 + the interior medium, high 16 bits = 1 + the exterior
 * medium, 0 = none (Shape::m_interiorMedium / m_exteriorMedium); a word other than 0 makes the primitive a medium transition
 * (Intersection::isMediumTransition), at which a path that leaves along d continues in the exterior medium when dot(d, geometric normal)
 * > 0, else in the interior one (getTargetMedium).  tri_media, sphere_media, shape_media: one word per triangle, per ppg_scene.spheres
 * entry, per ppg_set_shapes entry; NULL = all 0.  camera_medium: 1 + the medium the sensor lies in, 0 = none.
 * Random numbers, per medium event, in the reference's order: sampleDistance 1 (+ 1 under balance when the first falls below the
 * sampling weight), the emitter sample 2, the phase sample 2, Russian roulette 1.  exp / log are include/ppg_detmath.h's.
 * ppg_set_scene returns PPG_ERR_INVALID, names the entry in ppg_last_error and leaves the previous scene set for: more than 65535 media;
 * binding counts that differ from the scene's (n_tri_media / n_sphere_media / n_shape_media against n_triangles, n_spheres and the
 * ppg_set_shapes list, each checked when its array is given); a medium index out of range; a coefficient that is negative or not finite;
 * an unknown strategy or phase; channel > 2; g outside (-1, 1); sampling_density <= 0 or not finite under manual; sampling_weight
 * outside [0, 1] and not -1; a non-zero reserved word.
 * A scene with a media list that binds at least one medium (a non-zero word or camera_medium) runs the "media" kernels (csrc:
 * PPG_MEDIA), whatever else it holds; a list without a binding renders exactly as no list does.  Sharded renders (ppg_set_shard with
 * world > 1) refuse such a scene.  ppg_render_fields does not see media (Mitsuba's field integrator does not).  The CPU oracle does not
 * know media: they are pinned against a float64 restatement item by item, by reduction and by closed forms.
 * ---------------------------------------------------------------------------------------------- */
enum { PPG_MEDIUM_BALANCE = 0, PPG_MEDIUM_SINGLE = 1, PPG_MEDIUM_MANUAL = 2 };
enum { PPG_PHASE_ISOTROPIC = 0, PPG_PHASE_HG = 1 };
typedef struct ppg_medium {
    float sigma_a[3], sigma_s[3]; /* already scaled                                                  offset  0, 12 */
    int32_t strategy;             /* PPG_MEDIUM_*                                                            24 */
    int32_t channel;              /* single: 0..2, or < 0 = the channel with the smallest sigmaT              28 */
    float sampling_density;       /* manual                                                                  32 */
    float sampling_weight;        /* [0, 1], or -1 = derive                                                  36 */
    int32_t phase;                /* PPG_PHASE_*                                                             40 */
    float g;                      /* hg                                                                      44 */
    uint32_t _reserved[4];        /* must be 0                                                               48 */
} ppg_medium;                     /* 64 bytes */
typedef struct ppg_media {
    uint32_t n_media;
    uint32_t camera_medium;       /* 1 + index, 0 = none */
    const ppg_medium *media;      /* [n_media] */
    uint32_t n_tri_media, n_sphere_media, n_shape_media;  /* entries of the three arrays below (ignored where the array is NULL) */
    uint32_t _reserved;           /* must be 0 */
    const uint32_t *tri_media;    /* [n_triangles] or NULL */
    const uint32_t *sphere_media; /* [n_spheres] or NULL */
    const uint32_t *shape_media;  /* [entries of ppg_set_shapes] or NULL */
} ppg_media;
int ppg_set_media(ppg_ctx *ctx, const ppg_media *media);

/* ------------------------------------------------------------------------------------------------
 * Heterogeneous participating media (medium/heterogeneous.cpp with method = woodcock, its default) over constant and grid volumes
 * (volume/constvolume.cpp, volume/gridvolume.cpp, float32 data): a density field and an albedo field, delta (Woodcock) tracking for
 * sampleDistance (heterogeneous.cpp:613-662) and the two-run tracking estimate for evalTransmittance (:553-585), which draws random
 * numbers from the path's own stream, in the reference's order.
 * One more side list: call before ppg_set_media / ppg_set_scene; ppg_set_scene validates and consumes it together with the media list;
 * the context keeps it until it is replaced (NULL, or n_entries = 0, clears it); PPG_ERR_STATE between ppg_begin_render and
 * ppg_end_render.  ppg_medium and ppg_media stay as they are: an entry here names a medium of ppg_media's list and makes it heterogeneous.
 * Of such a medium sigma_a, sigma_s, strategy, channel, sampling_density are not read and must be 0, sampling_weight 0 or -1; phase and g
 * hold as for a homogeneous medium.
 *   volumes   PPG_VOLUME_CONST: `value` (channels = 1: value[0]; 3: an RGB triple).  PPG_VOLUME_GRID: res = (x, y, z) nodes, channels 1 or
 *             3, float32 data in the order ((z * res[1] + y) * res[0] + x) * channels + c, the data's box aabb_min / aabb_max in the
 *             volume's own space and to_world (row-major 4x4, affine).  The lookup is trilinear between the nodes and 0 outside them
 *             (gridvolume.cpp:337-388).  ppg_set_scene derives worldToGrid = scale((res - 1) / extents) * translate(-aabb_min) *
 *             to_world^-1 (gridvolume.cpp:188-201) and the world-space box of the eight transformed corners.
 *   entries   medium = index into ppg_media.media; density = a one-channel volume; albedo = a three-channel volume; scale multiplies the
 *             density.  maxDensity = scale * (1 for a grid: Mitsuba's tracking assumes a grid density of at most 1; the value for a
 *             const volume) and its inverse are derived as heterogeneous.cpp:239-242 does.  A const density has the reference's default
 *             box, on which AABB::rayIntersect answers (-inf, +inf) — and false for a ray with a zero direction component.
 * ppg_set_scene returns PPG_ERR_INVALID, names the entry in ppg_last_error and leaves the previous scene set for: a list without a media
 * list; an index out of range; a medium named twice; a density volume with channels != 1 or an albedo volume with channels != 3; an
 * unknown kind; a res component below 2; an empty or non-finite data box; a singular or non-finite to_world; a scale that is not finite
 * and positive; a const density that is not finite and positive; a grid density texel outside [0, 1] or not finite; an albedo value
 * outside [0, 1] or not finite; a coefficient of the named medium that is not 0; a non-zero reserved word; a grid without data; and a grid
 * density whose expected tracking length is too long: scale * the diagonal of its world box above PPG_HETMEDIUM_MAX_MEAN_STEPS majorant
 * free paths (one segment's loop would run that many steps per lane).  Sharded renders refuse such a scene as they refuse every medium.
 * A scene that binds a heterogeneous medium runs the "hetmedia" kernels (csrc: PPG_HETMEDIA), whatever else it holds.
 * ---------------------------------------------------------------------------------------------- */
enum { PPG_VOLUME_CONST = 0, PPG_VOLUME_GRID = 1 };
#define PPG_HETMEDIUM_MAX_MEAN_STEPS 4096.0f
typedef struct ppg_volume {
    int32_t kind;                 /* PPG_VOLUME_*                                                     offset   0 */
    int32_t channels;             /* 1 or 3                                                                    4 */
    float value[3];               /* const                                                                     8 */
    int32_t res[3];               /* grid: nodes along x, y, z                                                20 */
    float aabb_min[3], aabb_max[3]; /* grid: the data's box                                               32, 44 */
    float to_world[16];           /* grid: row-major                                                          56 */
    uint32_t _reserved[2];        /* must be 0                                                               120 */
    const float *data;            /* grid: [res[2] * res[1] * res[0] * channels]                             128 */
} ppg_volume;                     /* 136 bytes */
typedef struct ppg_medium_volumes {
    uint32_t medium;              /* index into ppg_media.media                                                0 */
    uint32_t density, albedo;     /* indices into ppg_media_volumes.volumes                                 4, 8 */
    float scale;                  /*                                                                          12 */
    uint32_t _reserved[4];        /* must be 0                                                                16 */
} ppg_medium_volumes;             /* 32 bytes */
typedef struct ppg_media_volumes {
    uint32_t n_volumes, n_entries;      /*                                                                  0, 4 */
    const ppg_volume *volumes;          /* [n_volumes]                                                         8 */
    const ppg_medium_volumes *entries;  /* [n_entries]                                                        16 */
    uint32_t _reserved[4];              /* must be 0                                                          24 */
} ppg_media_volumes;                    /* 40 bytes */
int ppg_set_media_volumes(ppg_ctx *ctx, const ppg_media_volumes *volumes);

/* ------------------------------------------------------------------------------------------------
 * Rendering.  ppg_render() is GuidedPathTracer::render() (GP:1516-1585, IH:74-75) in one call.
 * The stepwise calls expose its phases so a multi-GPU driver can all-reduce the SD-tree statistics
 * between ppg_render_passes() and ppg_build_sdtree(); ppg_render() is exactly their composition
 * (renderSPP GP:1342-1426 / renderTime GP:1434-1514).
 * ---------------------------------------------------------------------------------------------- */
int ppg_render(ppg_ctx *ctx);

int ppg_begin_render(ppg_ctx *ctx);                       /* GP:1519-1550: new STree(aabb), buffers, m_iter = 0 */
int ppg_begin_iteration(ppg_ctx *ctx, int32_t is_final);  /* GP:1378-1381: m_isFinalIter, film->clear(), resetSDTree() GP:1108-1113 */
int ppg_set_final(ppg_ctx *ctx, int32_t is_final);        /* GP:1409 / 1492: m_isFinalIter = true before the FINAL passes */
int ppg_set_do_nee(ppg_ctx *ctx, int32_t do_nee);         /* GP:1362 m_doNee */
int ppg_render_passes(ppg_ctx *ctx, int32_t n_passes, ppg_pass_stats *stats); /* performRenderPasses GP:1210-1329 */
int ppg_build_sdtree(ppg_ctx *ctx, ppg_tree_stats *stats);                    /* buildSDTree GP:1115-1189 */
int ppg_end_iteration(ppg_ctx *ctx);                      /* GP:1417-1422: optional dump, ++m_iter */
int ppg_end_render(ppg_ctx *ctx);                         /* GP:1567-1582: inverse-variance combination into the film */

/* Integrator::cancel() (IH:84, GP:1643-1648).  Thread-safe; the running ppg_render / ppg_render_passes
   call returns PPG_ERR_CANCELLED.  The request is sticky: with no render under way — the context exists and its scene is still being set
   up, seconds of BVH build — it cancels the NEXT one (ppg_begin_render / ppg_render return PPG_ERR_CANCELLED at once and consume it).  A
   request a render has acted on is spent and does not reach the render after it. */
int ppg_cancel(ppg_ctx *ctx);
/* Device blocks released by contexts (buffer growth, ppg_destroy) are kept by the library — at most a third of the device's memory —
   and handed to the next allocation that fits, of this or another context (hipMalloc / hipFree of hundreds of MB are synchronous,
   millisecond-scale calls).  This gives the kept blocks of `device` back to the driver; the library also does so by itself when an
   allocation fails. */
int ppg_release_cached_memory(int32_t device);

/* Film read-back: weight-normalised RGB, row-major [height][width][3] (hdrfilm develop, fmtconv.cpp:1036-1044). */
int ppg_read_film(ppg_ctx *ctx, float *rgb);
/* Per-pixel variance estimate of the last ppg_render_passes (m_varianceBuffer, GP:1298-1314), [h][w][3]. */
int ppg_read_variance(ppg_ctx *ctx, float *rgb);

/* dumpSDTree (GP:1191-1208) in the byte format of DTreeWrapper::dump (GP:699-711), readable by
   visualizer/src/main.cpp:142-176.  camera_matrix = row-major 4x4 world transform. */
int ppg_dump_sdtree(ppg_ctx *ctx, const char *path);

/* ------------------------------------------------------------------------------------------------
 * Loading a dumped SD-tree (HIP library only): train once, render many.  The file is what ppg_dump_sdtree, the dumpSDTree property, the
 * reference's own dumpSDTree or the CPU oracle wrote; the context continues from it as if it had trained the tree itself — a final
 * iteration from another camera or at a higher sample count, or further training iterations.
 *
 * When: after ppg_begin_render, with no iteration open (before ppg_begin_iteration, or after ppg_build_sdtree); otherwise PPG_ERR_STATE.
 * With a shard set (ppg_set_shard, world > 1) the call is refused by name (PPG_ERR_INVALID, "not supported yet").
 *
 * Afterwards the context is in the state that ppg_build_sdtree + ppg_end_iteration of iteration opts->iter - 1 leave: S-tree, leaf
 * headers, lookup grid, sampling D-trees, is_built, and m_iter / m_passesRendered as given.  Every call works from there unchanged:
 * ppg_begin_iteration (refines the S-tree by the loaded weights, resets the building trees from the loaded sampling trees),
 * ppg_render_passes, ppg_build_sdtree, ppg_dump_sdtree, the ppg_sdtree_read_* readers, ppg_query_pdf / ppg_query_sample.  Until that
 * ppg_begin_iteration the building trees read as the sampling trees' topology with empty accumulators.
 *
 * The S-tree is not in the file: it is rebuilt from the leaf boxes.  From the context's tree box (ppg_sdtree_info.aabb_min / aabb_max) and
 * axis 0, with the dump's own float arithmetic (size[axis] /= 2; child 1: p[axis] += size[axis]; next axis = (axis + 1) % 3), the next
 * leaf of the file either IS the region (exact float equality), lies inside it (the region is split), or the region is a hole.  S-tree
 * nodes are numbered in preorder; the numbering of the context that wrote the file cannot be recovered, and nothing depends on it.
 *
 * What the format loses:
 *   - statistical weights are truncated to integers (they are integers under the nearest spatial filter, fractional under the others);
 *   - `mean` stands in for the D-tree's sum: sum = mean * (4 pi * weight), up to 4 ulp from the sum that was dumped;
 *   - there is no optimiser state: with bsdfSamplingFractionLoss != none the learned fraction restarts at 0.5 in every leaf;
 *   - leaves of weight 0 are not in the file: each maximal region without a leaf becomes ONE leaf with an empty D-tree (one node, four zero
 *     sums, weight 0), which samples uniformly as the leaves it replaces did.
 * With the nearest filters and no loss a render continued from a file is therefore bit-identical to the uninterrupted one (film, variance,
 * pass statistics, further dumps); with the other settings it is a valid, slightly different guiding distribution.
 *
 * Refusals — all decided on the host (csrc/ppg_sdt_load.h) before a byte is uploaded or a kernel launched; the context keeps the tree it
 * had and stays usable; ppg_last_error names the leaf and the file offset.  PPG_ERR_INVALID: a file that cannot be read; a truncated file
 * or trailing bytes that do not form a leaf; numNodes 0, above 65536 or beyond the bytes that remain; a child index >= numNodes, not above
 * its parent's, or referenced twice; a node no node refers to; a sum that is negative or not finite; a mean or box that is not finite (or
 * a size <= 0); a D-tree deeper than 20 levels; a leaf box that is not a region of this context's tree box ("the tree was trained on
 * another scene"); leaves out of depth-first order or overlapping; opts->iter outside 0 .. 30, a negative passes_rendered.  PPG_ERR_NOMEM:
 * 2^27 S-tree nodes or 2^32 sampling nodes; with the box spatial filter an S-tree deeper than PPG_STREE_MAX_DEPTH (ppg_testhooks.h).
 * Not offered by the C++ driver, the .ppgs tools, the Mitsuba plug-in or the CPU oracle.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_sdtree_load {
    int32_t iter;            /* m_iter of the state the file was dumped from (ppg_sdtree_info.iter of the dumping context) */
    int32_t passes_rendered; /* m_passesRendered there: sample indices go on from passes_rendered * sppPerPass */
    int32_t _reserved[2];    /* 0 */
} ppg_sdtree_load;
int ppg_load_sdtree(ppg_ctx *ctx, const char *path, const ppg_sdtree_load *opts /* NULL: zeros */);

/* ------------------------------------------------------------------------------------------------
 * Feature buffers of the first hit (HIP library only): Mitsuba's `field` integrator (mitsuba/src/integrators/misc/field.cpp:122-175) —
 * what a denoiser wants beside the radiance: albedo, normals, position, depth — one image per requested field, filtered with the film's
 * reconstruction filter (ppg_set_rfilter) exactly as the radiance is.
 *
 * When: after ppg_set_scene and not between ppg_begin_render and ppg_end_render (PPG_ERR_STATE).  The call reads the scene, the camera,
 * the lens, the film's filter and the configured seed and changes nothing of the context — no film, image, SD-tree, record or RNG state —:
 * a render before or after it is bit-identical to one without it.  A context with a shard (ppg_set_shard) still renders the WHOLE film's
 * fields: they cost a handful of primary rays, and every rank then holds the same bits.
 *
 * Sample j (0 .. spp - 1) of pixel p is the camera ray the render gives that pixel for sample index first_sample + j: the key is
 * ppg_path_key(seed, p, first_sample + j) (include/ppg_rng.h), dimensions 0 and 1 the position in the pixel, 2 and 3 the aperture point
 * of a thin lens; mint and maxt come from the clip planes.  A sample whose ray leaves the scene has the field's `undefined` value
 * (field.cpp:96-101; any float, NaN included).  Where the ray hits (field.cpp:130-169):
 *   POSITION      its.p
 *   REL_POSITION  its.p in camera space (field.cpp:134-139): the inverse of ppg_camera.camera_to_world, computed once on the host in
 *                 double from the camera's floats and rounded to float, applied as Transform::operator()(Point)
 *   DISTANCE      its.t in all three channels
 *   GEO_NORMAL, SH_NORMAL   its.geoFrame.n, its.shFrame.n.  Bump and normal maps do not enter: they act inside the BSDF, as in Mitsuba.
 *   UV            (u, v, 0): on a triangle with texture coordinates their interpolation, on a triangle without them the barycentrics
 *                 (b1, b2) (skdtree.h:403-410) whether or not the material reads a texture, on spheres, disks and cylinders (0, 0) (their
 *                 parameterisation is not computed: no BSDF on them reads a texture).  The XML loaders keep a mesh's coordinates only
 *                 where its BSDF reads them; elsewhere a loaded mesh shows barycentrics.
 *   PRIM_INDEX    the primitive's index in the scene description as a float in all three channels: the triangles in ppg_scene order (not
 *                 the BVH's leaf order), then the spheres, then the shapes of ppg_set_shapes.  Mitsuba counts per shape; the loaders
 *                 flatten shapes, so this scene-wide index is the only one there is, and `shapeIndex` is not offered.
 *   ALBEDO        BSDF::getDiffuseReflectance(its).  diffuse, roughdiffuse, phong: the diffuse reflectance — the bitmap of `texture`'s low
 *                 half at the hit's uv where there is one, else the constant (diffuse.cpp:106, roughdiffuse.cpp:124, phong.cpp:109).
 *                 plastic: that times 1 - fresnelDiffuseReflectance(eta) (plastic.cpp:195, 219-221).  roughplastic: the diffuse
 *                 reflectance WITHOUT roughplastic.cpp:309-315's factor Ftr — a deviation: the external rough-transmittance table's
 *                 diffuse value is not part of ppg_scene.rtrans.  Conductors, dielectrics, thindielectric, difftrans, null and the mirror:
 *                 0, they have no diffuse reflection (bsdf.cpp:82-86).  PPG_MAT_TWOSIDED, bump and normal maps: the nested value
 *                 (twosided.cpp:198-203, bumpmap.cpp:108, normalmap.cpp:80); a coat (ppg_set_coatings): the coated BSDF's value.
 *                 PPG_MAT_MASK: opacity (its bitmap where a slot names one) times the nested value — an own rule: mask.cpp has no
 *                 override, and BSDF's default would evaluate the nested diffuse lobe at normal incidence, 0 for roughdiffuse.
 *                 A scene with a blended material (ppg_set_blends) is refused when ALBEDO is among the fields ("albedo: blendbsdf /
 *                 mixturebsdf materials are not supported yet"); every other field works on such scenes.
 *
 * The image (ImageBlock::put with the film's filter: table, radius, border B and footprint clipping of ppg_set_rfilter; the default box is
 * the sample's own pixel with weight 1).  Summation goes by pass, then by tap, in the order (j, dy, dx): for j = 0 .. spp - 1 ascending a
 * sample pass, then a resolve pass in which each target pixel t adds w * V per channel and w to its accumulators over its taps dy = -B .. B
 * and within each dy dx = -B .. B; the tap (dx, dy) is source pixel t - (dx, dy)'s sample j, if that pixel is inside the film and t inside
 * that sample's clipped footprint.  At the end out = sum * (w != 0 ? 1 / w : 0).  No atomics: the result does not depend on the launch
 * shape.
 *
 * PPG_ERR_INVALID: a NULL pointer, n_fields 0 or above PPG_MAX_FIELDS, an unknown field, spp outside 1 .. 65536, the blend case.
 * Not offered by the C++ driver, the .ppgs container (they carry scenes, not requests), the Mitsuba plug-in or the CPU oracle.
 * ---------------------------------------------------------------------------------------------- */
enum { PPG_FIELD_POSITION = 0, PPG_FIELD_REL_POSITION = 1, PPG_FIELD_DISTANCE = 2, PPG_FIELD_GEO_NORMAL = 3,
       PPG_FIELD_SH_NORMAL = 4, PPG_FIELD_UV = 5, PPG_FIELD_ALBEDO = 6, PPG_FIELD_PRIM_INDEX = 7 };
#define PPG_MAX_FIELDS 8
typedef struct ppg_fields {
    uint32_t n_fields;                       /* 1 .. PPG_MAX_FIELDS */
    int32_t  field[PPG_MAX_FIELDS];          /* PPG_FIELD_*, repeats allowed */
    float    undefined[PPG_MAX_FIELDS][3];   /* field.cpp:96-101: the value of a sample whose ray leaves the scene; any float, NaN included */
    uint32_t spp;                            /* samples per pixel, 1 .. 65536 */
    uint32_t first_sample;                   /* sample index of the first one */
} ppg_fields;
int ppg_render_fields(ppg_ctx *ctx, const ppg_fields *f, float *out /* [n_fields][height][width][3] */);

/* ------------------------------------------------------------------------------------------------
 * SD-tree access (parity tests, multi-GPU reduction, visualisation).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ppg_sdtree_info {
    uint32_t n_stree_nodes;
    uint32_t n_leaves;
    uint64_t n_sampling_nodes; /* total quadtree nodes of all sampling D-trees (shared blocks counted once) */
    uint64_t n_building_nodes; /* total quadtree nodes of all building D-trees */
    float aabb_min[3], aabb_max[3]; /* cubified, GP:857-859 */
    int32_t iter;
    int32_t is_built;
} ppg_sdtree_info;

int ppg_sdtree_info_get(ppg_ctx *ctx, ppg_sdtree_info *info);

/* S-tree nodes in the reference's numbering (STreeNode, GP:740-845): per node axis, children[2]
   (0,0 for a leaf).  Arrays sized n_stree_nodes. */
int ppg_sdtree_read_stree(ppg_ctx *ctx, int32_t *axis, uint32_t *children /* [n*2] */);

/* Per S-tree node D-tree headers (only meaningful for leaves).  which: 0 = sampling, 1 = building.
   offset = first node of that tree in the node arrays read by ppg_sdtree_read_dtree_nodes. */
int ppg_sdtree_read_dtree_headers(ppg_ctx *ctx, int32_t which, uint64_t *offset, uint32_t *num_nodes,
                                  int32_t *max_depth, float *sum, double *stat_weight);

/* Quadtree nodes (QuadTreeNode, GP:158-371) of all D-trees of one kind, concatenated.
   sums [n*4]: sampling → the float sums; building → the accumulated sums converted to float.
   children [n*4] (uint16, 0 = leaf slot).  fixed_sums may be NULL; building only: the raw 2^-PPG_FIXED_SHIFT
   fixed-point accumulators. */
int ppg_sdtree_read_dtree_nodes(ppg_ctx *ctx, int32_t which, float *sums, uint16_t *children, uint64_t *fixed_sums);

/* learned BSDF sampling fraction state per S-tree node (AdamOptimizer::State, GP:116-124): theta only */
int ppg_sdtree_read_adam(ppg_ctx *ctx, float *theta);

/* Device pointers to the accumulate-only statistics of the *building* SD-tree, for the per-iteration
   all-reduce(sum) of a multi-GPU render.  Both arrays are int64/uint64 fixed-point,
   so an integer sum is exact and order independent.  Valid until the next ppg_begin_iteration. */
int ppg_sdtree_stat_buffers(ppg_ctx *ctx, void **dev_sums, uint64_t *n_sums, void **dev_weights, uint64_t *n_weights);
/* Device pointers to the film accumulators (float RGB sums + sample counts), for the final gather. */
int ppg_film_buffers(ppg_ctx *ctx, void **dev_rgb_sum /* float[h*w*3] */, void **dev_weight /* float[h*w] */);
/* Device pointers to image / squared image of the current ppg_render_passes for the variance reduction:
   call between ppg_render_passes_nostat() and ppg_finish_passes() when sharded. */
int ppg_image_buffers(ppg_ctx *ctx, void **dev_image /* float[h*w*3] */, void **dev_sq_image /* float[h*w*3] */,
                      void **dev_weight /* float[h*w] */);
int ppg_render_passes_nostat(ppg_ctx *ctx, int32_t n_passes); /* GP:1217-1286 only */
int ppg_finish_passes(ppg_ctx *ctx, ppg_pass_stats *stats);   /* GP:1288-1328 only */

/* ------------------------------------------------------------------------------------------------
 * Final iteration: groups of passes.
 *
 * In the final iteration nothing is recorded (GP:2150-2154, !m_isFinalIter) and it holds at least half of a render's samples
 * (GP:1367-1374); the sampler is keyed by (pixel, sample index), so its passes are independent of each other.  A sharded render therefore
 * deals them to the ranks WHOLE — all pixels — instead of splitting every pass by tiles: the tail of a batch of unbounded paths lasts as
 * long as its longest path (a guided path survives a bounce with probability 0.99, GP:2124-2139), a term that does not shrink with the
 * number of ranks when every rank runs every batch, and does when a rank runs every world-th batch.
 * So that the film is the same on one GPU and on N, bit for bit, the float sums are given one association:
 *   - the n passes of a ppg_render_passes() call made with the final flag set (budgetType = spp) form groups of
 *     ppg_final_group_passes(n) = 16 * ceil(n / 1024) consecutive passes (at most 64 groups);
 *   - a group's samples are summed per pixel in sample order, from zero, into the group's partial (image, squared image, weight);
 *   - the call's image / squared image / weights and the iteration's film are the partials added in group order.
 * Sharded: WHO renders a group does not enter the sums, so it is chosen by count.  With at least two groups per rank (groups >= 2 * world)
 * group g is rendered by rank g % world over the whole film; with fewer — a 13-pass final iteration is ONE group, one of 64 passes four —
 * every rank renders every group on its own tiles (ppg_set_shard), or most ranks would idle through half of the render's samples.  Either
 * way, between ppg_render_passes_nostat() and ppg_finish_passes() the host all-reduces (sum, float) the n_floats at `dev` —
 * [film 3 n][film weights n][groups x (image 3 n, squared image 3 n, weights n)], n = pixels; every pixel of a slot is non-zero on one rank
 * only and the film head (the tile-sharded training passes an `automatic` render adds to the same iteration, GP:1400-1405) has disjoint
 * supports, so the sums are exact — and calls ppg_final_partials_commit().  Afterwards image and film are complete on every rank: no
 * ppg_image_buffers / ppg_film_buffers exchange for this iteration.  n_floats = 0: not a sharded final iteration (one rank, or a time
 * budget), exchange the image buffers as usual.  n_floats depends only on the film size and the pass count (4 n + groups * 7 n): a rank
 * that failed can still join the collective, with zeros.
 * ---------------------------------------------------------------------------------------------- */
/* budgetType = seconds in a sharded render: every decision the reference takes by its clock (GP:1259-1262 inside performRenderPasses,
   GP:1434-1514 in renderTime) must come out the same on all ranks, or they would render different numbers of passes and their collectives
   would stop matching.  The stop hook is asked after every batch of passes with this rank's own decision (elapsed whole seconds > budget) and
   returns the one all ranks follow — rank 0's.  The exchange behind it also carries the ranks' status words (host/rccl_reducer.h
   stopDecision: one all-reduce of {decision, status}): a rank that was cancelled asks the hook once more before it leaves the batch loop —
   with local_stop = PPG_STOP_CANCELLED (2) instead of a 0 / 1 decision, so that the host sets its status word even when the cancel did not
   come through the host's own cancel() —, so it meets the others in the exchange they are in, every rank stops there, and the image exchange
   that follows aborts the render on all of them.  The host loop passes the times it measures through a broadcast of rank 0's. */
#define PPG_STOP_CANCELLED 2
typedef int (*ppg_stop_hook)(void *user, int local_stop);
int ppg_set_stop_hook(ppg_ctx *ctx, ppg_stop_hook hook, void *user);
/* The HIP stream (hipStream_t) the context's kernels run on.  A reducer that enqueues its collectives on it needs no host synchronisation
   between an exchange and the library call that consumes its result: the round hook's all-to-all and all-gather are followed, in stream
   order, by the sort / apply / commit kernels. */
int ppg_exchange_stream(ppg_ctx *ctx, void **hip_stream);
int32_t ppg_final_group_passes(int32_t n_passes);
int ppg_final_partials(ppg_ctx *ctx, void **dev /* float[n_floats] */, uint64_t *n_floats);
int ppg_final_partials_commit(ppg_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * Footprint hook: a filtered film (ppg_set_rfilter) in a render sharded by tiles.
 *
 * The footprint is indexed by SOURCE pixel: slot (tap, c) of source s holds what s adds to target s + (dx, dy), tap = (dy + B) * (2B + 1)
 * + (dx + B), |dx|, |dy| <= B (the filter's border, at most 3), c = image RGB, squared image RGB, weight.  A BORDER SLOT is a pair (s, tap)
 * whose target lies inside the film AND on a tile of another rank than s's tile (owner of a tile = tile % world, tiles of tile_size²
 * pixels in row-major order; with tile_size < B the target may lie several tiles away).  The set depends on (width, height, tile_size,
 * world, B) only, so every rank numbers the same M slots alike: tap by tap (tap ascending) and, within a tap, by source pixel in row-major
 * order — the lanes of a wave touch consecutive source pixels of one tap.  The halo buffer is channel-major: float halo[7][M],
 * halo[c * M + m] = channel c of slot m.  ppg_footprint_halo_floats() = 7 M; 0 for world <= 1 or border < 1 (the default box keeps its
 * own-pixel film and has no footprint).
 *
 * Whenever a footprint is complete the library packs the border slots of ITS sources into the zeroed halo buffer (zeroing them in the
 * footprint), synchronises its stream and calls the hook, which all-reduces (sum, float) the n_floats at dev_halo in place together with
 * the ranks' status words — on the stream of ppg_exchange_stream, or on another one it synchronises before it returns — and returns
 * non-zero if any rank reported a failure.  Every float is non-zero on one rank at most: the sum is exact.  The library then writes the
 * slots whose TARGET it owns into its footprint and resolves its own target pixels only, taps in the usual order from zero; all other
 * pixels of image / squared image / weights / film (or of a final group's slot) stay untouched, so the image, film and final-partials
 * exchanges keep their disjoint supports.  The hook is called
 *   - once at the end of every ppg_render_passes_nostat() call that is not rendered in final groups (training passes, rounds by region, a
 *     seconds budget), after the last stragglers were flushed;
 *   - once per group in a final call (final flag, budgetType = spp) whose groups are rendered by tiles (groups < 2 * world): the groups are
 *     then rendered one at a time, each one's stragglers flushed before its exchange;
 *   - never at world = 1, with the default box, or in a final call whose groups are dealt whole to the ranks (a rank renders the whole film
 *     there and resolves it as one GPU does).
 * The number of calls in a ppg_render_passes_nostat() call thus depends only on what every rank knows.  A rank that is cancelled or fails
 * before a due call still makes that ONE next call, with a zeroed buffer (dev_halo may be NULL if it could not be allocated: zeros of the
 * hook's own) and local_status != 0; the hook then returns non-zero on all ranks, none of them makes a further call in this
 * ppg_render_passes_nostat(), and all return an error — to meet again in the image / final-partials exchange that follows.
 * ppg_set_footprint_hook comes BEFORE the filter and the shard meet (ppg_set_rfilter / ppg_set_shard refuse the combination without it);
 * clearing it (NULL) while a filter other than the default box and world > 1 are both set is PPG_ERR_INVALID.
 * ---------------------------------------------------------------------------------------------- */
typedef int (*ppg_footprint_hook)(void *user, void *dev_halo /* float[n_floats], device memory */, uint64_t n_floats, int32_t local_status);
int ppg_set_footprint_hook(ppg_ctx *ctx, ppg_footprint_hook hook, void *user);
uint64_t ppg_footprint_halo_floats(int32_t width, int32_t height, int32_t tile_size, int32_t world, int32_t border);

/* ------------------------------------------------------------------------------------------------
 * Learning the BSDF sampling fraction (bsdfSamplingFractionLoss = "kl" | "var"; AdamOptimizer GP:69-133,
 * DTreeWrapper::optimizeBsdfSamplingFraction GP:672-697).
 *
 * The reference calls optimizeBsdfSamplingFraction() for every committed record under a per-D-tree spin-lock, in the order
 * in which its worker threads happen to arrive: AdamOptimizer::append() accumulates gradient * weight and takes one step
 * whenever the accumulated weight exceeds batchSize = 1 (GP:85-95), the gradient being evaluated at the variable's value at
 * that moment.  That order is not reproducible (not even between two runs of the reference).  This build keeps the rule and
 * fixes the order:
 *   - the n passes of a ppg_render_passes() call (= the training passes of an iteration) are rendered in ROUNDS of
 *     ppg_adam_round_passes(.., n) consecutive passes — at least two rounds per iteration from the second iteration on, so that
 *     the fractions learned from the first half already steer the second (measured on cbox-improved: variance of iterations
 *     2..6 within noise of the literal rule).  All paths of a round are sampled with the fractions in effect
 *     at its start;
 *   - at the end of the round every record that reached DTreeWrapper::record with product > 0 is applied to its D-tree with
 *     exactly the reference's arithmetic (float, gradient at the current variable, append(), step()), D-tree by D-tree, in
 *     ascending order of the 64-bit key
 *         leaf << PPG_ADAM_LEAF_SHIFT | path << PPG_ADAM_CODE_BITS | code
 *     leaf = S-tree node of the D-tree; path = (sample index within the round) * width * height + pixel index;
 *     code = PPG_ADAM_CODE_VERTEX + i for path vertex i (Vertex::commit, GP:2150-2154), min(rRec.depth, PPG_ADAM_CODE_VERTEX - 1)
 *     for the direct-light vertex of next-event estimation (GP:1994-2010).  Keys are unique, so the order is total: a valid
 *     serialisation of the reference's critical sections that does not depend on wave scheduling, thread or GPU count.
 * What the fixed order costs (measured against the reference's own render logs): under the reference's rule the
 * variable follows the records of the last ~100 paths — of the image region being rendered —, which a value frozen for a round cannot; the
 * variance estimate of the EARLY iterations is up to twice the reference's on spaceship-improved (equal from iteration 6, 64 passes, on),
 * unaffected from iteration 2 on on kitchen-improved.  The oracle implements the literal rule too (PPGO_ADAM_SEQUENTIAL) and reproduces the
 * reference's logs with it to 1 - 4 %.
 * AdamOptimizer::State (incl. the partial batch) survives rounds, iterations and STree subdivision (GP:890) as in the reference.
 *
 * STRAGGLERS (round 6).  With maxDepth = -1 a guided path survives Russian roulette with probability 0.99 (GP:2124-2139): one path in
 * ten thousand runs for hundreds of bounces, and a round that waits for it before its records may be applied idles the GPU for
 * milliseconds — on every GPU of a sharded render alike.  The reference applies a path's records when that path happens to finish
 * (Vertex::commit at the end of Li, GP:2150-2154, under the lock of GP:719-737): records of long paths arrive late there too.  The rule
 * here, deterministic and independent of wave scheduling, batch size, thread and GPU count:
 *   - in a round whose record positions are known in advance (spatialFilter != box, no kick-start luminaire sampling in effect) of a
 *     render with maxDepth = -1, a path whose FINAL rRec.depth (the value Li adds to avgPathLength, GP:2147-2148) exceeds
 *     PPG_ADAM_DEFER_DEPTH is a straggler;
 *   - a straggler's optimiser records are applied with the NEXT round of the same ppg_render_passes() call — per D-tree after that
 *     round's own records: their keys carry PPG_ADAM_DEFER_PATH_BIT in the path field, so "ascending key order" says exactly that —,
 *     and those of the call's last round in a round of their own at the end of the call (the sharded render's round hook is called for
 *     it on every rank, with or without records);
 *   - nothing else moves: the straggler's splats reach the building tree before ppg_build_sdtree (integer sums: the same bits whenever
 *     they land), its radiance reaches image and film in its sample's place in the sums.
 * On KITCHEN one path in 10^4 is a straggler (16-pass round at 1280x720: 1 481 of 14.7 M); the product finishes them on a side stream
 * beside the next round's paths (ppg_hip.hip "Stragglers").  The oracle implements the same rule.
 * Limits: width * height * sppPerPass <= 2^(PPG_ADAM_PATH_BITS - 1) and at most 2^24 S-tree nodes while a loss is set.
 * ---------------------------------------------------------------------------------------------- */
#define PPG_ADAM_ROUND_MAX_PASSES 16
#define PPG_ADAM_ROUND_MAX_PATHS (1u << 24)
#define PPG_ADAM_CODE_BITS 13
#define PPG_ADAM_PATH_BITS 27
#define PPG_ADAM_LEAF_SHIFT (PPG_ADAM_CODE_BITS + PPG_ADAM_PATH_BITS)
#define PPG_ADAM_CODE_VERTEX 4096
#define PPG_ADAM_DEFER_DEPTH 64
#define PPG_ADAM_DEFER_PATH_BIT (1u << (PPG_ADAM_PATH_BITS - 1))   /* in the path field of the key: a straggler's record, applied one round late */
/* passes per round for a call that renders n_passes: the largest power of two <= min(PPG_ADAM_ROUND_MAX_PASSES, n_passes / 2)
   whose paths (passes * sppPerPass * pixels of the whole image, not of a shard) stay within PPG_ADAM_ROUND_MAX_PATHS; at least 1 */
int32_t ppg_adam_round_passes(int32_t spp_per_pass, int32_t width, int32_t height, int32_t n_passes);

/* Rounds by image REGION — an extension, off by default (regions = 0), for renders whose EARLY iterations must follow the reference's.
   Under the reference's rule the optimiser's variable follows the records of the last ~100 paths, i.e. of the image region its 16 threads are
   rendering; a variable frozen for a whole pass cannot, and the variance estimate of iterations 1 - 4 is up to twice the reference's
   (above).  With regions = R >= 2, in every ppg_render_passes() call of at most PPG_ADAM_REGION_MAX_PASSES passes that is rendered in rounds,
   a round is ONE pass over ONE of R groups of 32x32-pixel blocks — consecutive in the spiral order in which the reference's scheduler hands
   blocks out (ppg_spiral_block_ranks, include/ppg_detmath.h; group of block b = rank(b) * R / blocks) — and the optimiser is applied after
   every group: R rounds per pass.  Measured against the reference's own log of spaceship-improved: variance estimate
   of iterations 1 - 4 within 2 - 13 % with R = 16 (2x with R = 0).  The price: R rounds of pixels / R paths each instead of one round of
   1 - 8 passes — on one MI355X the early iterations of KITCHEN at 1280x720 take several times longer.  Keys, stragglers,
   sharding (a rank renders its tiles of a group; R hook calls per pass on every rank) as for any round.  R is clamped to the number of blocks. */
#define PPG_ADAM_REGION_MAX_PASSES 16
int ppg_set_adam_regions(ppg_ctx *ctx, int32_t regions);

typedef struct ppg_adam_record { /* one deferred optimizeBsdfSamplingFraction() call: DTreeRecord's fields it reads (GP:562-568) */
    uint64_t key;
    float product, wo_pdf, bsdf_pdf, dtree_pdf, statistical_weight, _pad;
} ppg_adam_record;             /* 32 bytes */

/* Round hook for multi-GPU rendering: called at the end of every round after this rank's records were collected and before
   they are applied.  The hook gathers the records of all ranks (ppg_adam_records → exchange → ppg_adam_records_replace) so that
   every rank applies the identical sequence and the learned fractions stay bit-identical across ranks — and equal to a
   single-GPU render, because the key order does not depend on the sharding.  Return non-zero to abort. */
typedef int (*ppg_pass_hook)(void *user);
int ppg_set_pass_hook(ppg_ctx *ctx, ppg_pass_hook hook, void *user);
/* Valid inside the hook only.  dev_records: this rank's records (device memory, unspecified order). */
int ppg_adam_records(ppg_ctx *ctx, void **dev_records /* ppg_adam_record[n] */, uint64_t *n);
/* Valid inside the hook only: the records to apply instead (device pointer, copied). */
int ppg_adam_records_replace(ppg_ctx *ctx, const void *dev_records, uint64_t n);

/* Sharded optimiser: ONE OWNER PER D-TREE.  The reference serialises the Adam steps per D-tree (its spin-lock, GP:719-737), so the
   D-trees can be dealt to the ranks: S-tree node `leaf` belongs to rank leaf / segment, segment = ceil(n_stree_nodes / world) —
   contiguous node ranges, so with the records in key order every owner's records are one contiguous run.  The hook is then called
   TWICE per round:
     phase 0  before the records are applied: ppg_adam_records_by_owner → all-to-all (every rank keeps 1 / world of the records
              instead of gathering all of them) → ppg_adam_records_replace with what this rank owns; it then sorts and applies only those;
     phase 1  after they were applied (only if phase 0 called ppg_adam_records_by_owner): ppg_adam_state → all-gather of the
              owners' segments, in place → ppg_adam_state_commit.
   Same records in the same key order at the owner as in the union ⇒ the same bits as the gather-everything scheme and as one GPU. */
int ppg_hook_phase(ppg_ctx *ctx, int32_t *phase);
/* phase 0: this rank's records in key order (device memory) and how many of them each of the `world` owners gets */
int ppg_adam_records_by_owner(ppg_ctx *ctx, int32_t world, void **dev_records /* ppg_adam_record[sum(counts)] */, uint64_t *counts /* [world] */);
/* phase 1: the optimiser's state of every S-tree node, 24 bytes each (theta, iter, m, v, batchGradient, batchAccumulation; GP:116-124),
   packed into a device array of world * segment entries; rank r's segment [r * segment, (r + 1) * segment) holds what it computed */
int ppg_adam_state(ppg_ctx *ctx, int32_t world, void **dev_state, uint64_t *segment);
int ppg_adam_state_commit(ppg_ctx *ctx); /* take the (gathered) array back into the tree */

/* Batched queries against the current *sampling* SD-tree (what Li does per vertex):
   pdf  = DTreeWrapper::pdf(dir) of the leaf containing p        (GP:623-625, 897-905)
   dirs = DTreeWrapper::sample(sampler) with the build's sampler keyed by (seed, i)  (GP:619-621) */
int ppg_query_pdf(ppg_ctx *ctx, uint32_t n, const float *positions, const float *dirs, float *pdf_out);
int ppg_query_sample(ppg_ctx *ctx, uint32_t n, const float *positions, uint64_t seed, float *dirs_out);

/* Kernel timing of the last ppg_render_passes, measured with HIP events on the stream the kernels
   run on: names[i] → accumulated milliseconds and launch count.  Used by bench.py's roofline block. */
typedef struct ppg_kernel_time { const char *name; double ms; uint64_t launches; uint64_t units; } ppg_kernel_time;
int ppg_kernel_times(ppg_ctx *ctx, ppg_kernel_time *out, uint32_t cap, uint32_t *n);
int ppg_enable_kernel_timing(ppg_ctx *ctx, int32_t enable);

#define PPG_FIXED_SHIFT 24 /* building sums / weights are accumulated as round(x * 2^24) in uint64 */

#ifdef __cplusplus
}
#endif
#endif /* PPG_H */
