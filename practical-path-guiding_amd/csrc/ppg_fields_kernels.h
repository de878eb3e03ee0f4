/*
 * ppg_fields_kernels.h — the kernels of ppg_render_fields (include/ppg.h "Feature buffers of the first hit"), included by the k_trace unit
 * of the top (lobes) family (ppg_inst.hip), which compiles every material and shape a scene may hold:
 *   k_fields_sample      one lane per pixel of the whole film — the 64 lanes of a wave are neighbouring pixels of a row, their primary rays
 *                        coherent —: the sample's camera ray (camera_ray, as k_generate), the closest hit, the intersection record, the
 *                        values of the requested fields, stored SoA per field and channel with the sample's film position next to them
 *   k_fields_resolve<B>  one lane per target pixel and field: gathers the taps of the film's reconstruction filter, border B, in the
 *                        order (dy, dx) and adds them to the accumulators in device memory.  No atomics.
 */
#ifndef PPG_FIELDS_KERNELS_H
#define PPG_FIELDS_KERNELS_H

#include "ppg_launch.h"

#if PPG_FAMILY == PPG_FAMILY_LOBES
__global__ __launch_bounds__(64) void k_fields_sample(DevScene S, FieldsRequest F, unsigned long long seed, unsigned int sample, const float *albedo_scale, float *vals,
                                                      float *pos) {
    extern __shared__ int fld_stack[];  // PPG_LDS_STACK rows of 64: the traversal stack columns, as k_debug_intersect sets them up
    const unsigned int n = (unsigned int)S.cam.width * (unsigned int)S.cam.height;
    const unsigned int pixel = blockIdx.x * 64u + threadIdx.x;
    if (pixel >= n) return;
    const unsigned int key = ppg_path_key(seed, pixel, sample);
    unsigned int dim;
    F3 o, d;
    float mint, maxt;
    camera_ray(S.cam, key, pixel, o, d, mint, maxt, dim);
    {   // samplePos (GP:1620) - 0.5, as k_film_filter recomputes it
        const int px = (int)(pixel % (unsigned int)S.cam.width), py = (int)(pixel / (unsigned int)S.cam.width);
        pos[pixel] = ((float)px + ppg_rand(key, 0u)) - 0.5f;
        pos[(size_t)n + pixel] = ((float)py + ppg_rand(key, 1u)) - 0.5f;
    }
    const Hit h = trace_closest4<false, true>(S, fld_stack + threadIdx.x, 64, o, d, mint, maxt);
    const bool hit = h.prim >= 0;
    F3 p = f3s(0.0f), rel = f3s(0.0f), gn = f3s(0.0f), sn = f3s(0.0f), alb = f3s(0.0f);
    float u = 0.0f, v = 0.0f, prim = 0.0f;
    if (hit) {
        Isect I;
        if (h.prim >= S.n_tris) {
            fill_isect_analytic(S, h, o, d, I);  // (u, v) = (0, 0): the parameterisation of spheres, disks and cylinders is not computed
            prim = (float)h.prim;                // spheres, then shapes, behind the triangles: the scene description's order
        } else {
            TexInfo X;
            X.tex = 0u; X.u = 0.0f; X.v = 0.0f;
            fill_isect_tex<true>(S, h, d, I, X);
            // its.uv (skdtree.h:403-410): the interpolated coordinates, or the barycentrics on a mesh without them — whatever the material reads
            u = h.u; v = h.v;
            if (S.uvs) {
                const float2 t0 = S.uvs[3 * (size_t)h.prim], t1 = S.uvs[3 * (size_t)h.prim + 1], t2 = S.uvs[3 * (size_t)h.prim + 2];
                if (tri_has_uvs(t0, t1, t2)) tri_uv_at(t0, t1, t2, f3(1 - h.u - h.v, h.u, h.v), u, v);
            }
            prim = (float)__float_as_int(S.tris[3 * (size_t)h.prim + 2].w);  // the index in ppg_scene, not the leaf order
        }
        p = I.p; gn = I.geoN; sn = I.n;
        rel = xf_point(F.w2c, I.p);
        if (F.albedo) {
            // BSDF::getDiffuseReflectance(its): the record's reflectance or its bitmap, times the type's factor (the host's table: 1 - fdrExt of a
            // plastic, 0 without a diffuse reflection), times a mask's opacity
            const float scale = albedo_scale[I.material];
            if (scale != 0.0f) {
                const float4 *m = S.materials + PPG_MAT_STRIDE * (size_t)I.material;
                const float4 a = m[0], row = m[5];
                alb = f3(a.x, a.y, a.z);
                const unsigned int tr = __float_as_uint(row.x) & 0xffffu, to = __float_as_uint(row.w);
                if (tr) { const float4 t = tex_eval_slot(S.textures, tr, u, v); alb = f3(t.x, t.y, t.z); }
                alb = alb * scale;
                if (__float_as_int(m[2].w) & PPG_MAT_MASK) {
                    const float4 e = m[4];
                    F3 op = f3(e.x, e.y, e.z);
                    if (to) { const float4 t = tex_eval_slot(S.textures, to, u, v); op = f3(t.x, t.y, t.z); }
                    alb = mul3(op, alb);
                }
            }
        }
    }
    for (int f = 0; f < F.n_fields; ++f) {
        F3 val = f3(F.undefined[f][0], F.undefined[f][1], F.undefined[f][2]);
        if (hit) {
            switch (F.field[f]) {
                case PPG_FIELD_POSITION: val = p; break;
                case PPG_FIELD_REL_POSITION: val = rel; break;
                case PPG_FIELD_DISTANCE: val = f3s(h.t); break;
                case PPG_FIELD_GEO_NORMAL: val = gn; break;
                case PPG_FIELD_SH_NORMAL: val = sn; break;
                case PPG_FIELD_UV: val = f3(u, v, 0.0f); break;
                case PPG_FIELD_ALBEDO: val = alb; break;
                default: val = f3s(prim); break;  // PPG_FIELD_PRIM_INDEX (the host has refused every other value)
            }
        }
        float *dst = vals + (size_t)f * 3 * n + pixel;
        dst[0] = val.x; dst[(size_t)n] = val.y; dst[2 * (size_t)n] = val.z;
    }
}

// Target pixel t, field blockIdx.y: over the taps dy = -B .. B and within each dy dx = -B .. B, the tap (dx, dy) is source pixel
// t - (dx, dy)'s sample of this pass, if that pixel is inside the film and t inside the sample's clipped footprint (ImageBlock::put,
// k_film_filter's rule); w * V per channel goes to sum[field][t][3] and — by the lanes of field 0 — w to wsum[t].
template <int B>
__global__ __launch_bounds__(256) void k_fields_resolve(FilmFilter ff, const float *vals, const float *pos, float *sum, float *wsum) {
    __shared__ float tab[32];
    if (threadIdx.x < 32) tab[threadIdx.x] = ff.table[threadIdx.x];
    __syncthreads();
    const int W = ff.W, H = ff.H;
    const size_t n = (size_t)W * (size_t)H;
    const unsigned int t = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (t >= n) return;
    const int tx = (int)(t % (unsigned int)W), ty = (int)(t / (unsigned int)W);
    const float r = ff.radius, scale = ff.scale;
    const float *V = vals + (size_t)f * 3 * n;
    float *acc = sum + ((size_t)f * n + t) * 3;
    float s0 = acc[0], s1 = acc[1], s2 = acc[2], sw = f == 0u ? wsum[t] : 0.0f;
    for (int dy = -B; dy <= B; ++dy) {
        const int sy = ty - dy;
        if (sy < 0 || sy >= H) continue;
#pragma unroll
        for (int dx = -B; dx <= B; ++dx) {
            const int sx = tx - dx;
            if (sx < 0 || sx >= W) continue;
            const size_t src = (size_t)sy * W + sx;
            const float posx = pos[src], posy = pos[n + src];
            const int ylo = max((int)ceilf(posy - r), 0), yhi = min((int)floorf(posy + r), H - 1);
            if (ty < ylo || ty > yhi) continue;
            const int xlo = max((int)ceilf(posx - r), 0), xhi = min((int)floorf(posx + r), W - 1);
            if (tx < xlo || tx > xhi) continue;
            const float wy = tab[min((int)fabsf(((float)ty - posy) * scale), 31)];
            const float w = tab[min((int)fabsf(((float)tx - posx) * scale), 31)] * wy;
            s0 += w * V[src]; s1 += w * V[n + src]; s2 += w * V[2 * n + src];
            sw += w;
        }
    }
    acc[0] = s0; acc[1] = s1; acc[2] = s2;
    if (f == 0u) wsum[t] = sw;
}

static void launch_fields_sample(const FieldsSampleLaunch &a) {
    const unsigned int n = (unsigned int)a.S.cam.width * (unsigned int)a.S.cam.height;
    hipLaunchKernelGGL(k_fields_sample, dim3((n + 63u) / 64u), dim3(64), (size_t)PPG_LDS_STACK * 64 * sizeof(int), a.stream, a.S, a.F, a.seed, a.sample, a.albedo_scale,
                       a.vals, a.pos);
}
static void launch_fields_resolve(const FieldsResolveLaunch &a) {
    const unsigned int n = (unsigned int)a.ff.W * (unsigned int)a.ff.H;
    const dim3 g((n + 255u) / 256u, (unsigned int)a.n_fields), b(256);
    switch (a.border) {
    case 0: hipLaunchKernelGGL(k_fields_resolve<0>, g, b, 0, a.stream, a.ff, a.vals, a.pos, a.sum, a.wsum); break;
    case 1: hipLaunchKernelGGL(k_fields_resolve<1>, g, b, 0, a.stream, a.ff, a.vals, a.pos, a.sum, a.wsum); break;
    case 2: hipLaunchKernelGGL(k_fields_resolve<2>, g, b, 0, a.stream, a.ff, a.vals, a.pos, a.sum, a.wsum); break;
    default: hipLaunchKernelGGL(k_fields_resolve<3>, g, b, 0, a.stream, a.ff, a.vals, a.pos, a.sum, a.wsum); break;
    }
}
#endif

// the launchers of this family, into its row
static void fill_fields_kernels(PathKernels &K) {
#if PPG_FAMILY == PPG_FAMILY_LOBES
    K.fields_sample = launch_fields_sample;
    K.fields_resolve = launch_fields_resolve;
#endif
}

#endif
