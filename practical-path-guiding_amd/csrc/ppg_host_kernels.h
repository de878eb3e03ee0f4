/*
 * ppg_host_kernels.h — the small kernels: everything that is not a large path kernel.  Only ppg_hip.hip launches them and only it includes
 * this header, so they are compiled once, not into every translation unit of ppg_inst.hip.  The order is that of a render (ppg_kernels.h).
 */
#ifndef PPG_HOST_KERNELS_H
#define PPG_HOST_KERNELS_H

#include "ppg_kernels.h"

// ------------------------------------------------------------------------------------------------
// k_generate — renderBlock's sample loop head (GP:1613-1630) + the camera ray of the sample (camera_ray, ppg_device.h)
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(PPG_BLOCK) void k_generate(PathState P, DevScene S, RenderParams R, Queues Q) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.n_paths; i += gridDim.x * blockDim.x) {
        unsigned int k = i % P.n_pix, j = i / P.n_pix;
        unsigned int pixel = P.pixels[k];
        const unsigned int sample = R.group_samples ? R.pass_index_spp + (j / R.group_samples) * R.group_stride + (j % R.group_samples) : R.pass_index_spp + j;
        unsigned int key = ppg_path_key(R.seed, pixel, sample);
        unsigned int dim;
        F3 o, d;
        float mint, maxt;
        camera_ray(S.cam, key, pixel, o, d, mint, maxt, dim);
        P.ray_o[i] = make_float4(o.x, o.y, o.z, mint);
        P.ray_d[i] = make_float4(d.x, d.y, d.z, maxt);
        P.thr[i] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        P.li[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        P.misc[i] = make_uint4(key, dim, 1u | FL_EMITTED_OK, 0u);
    }
}

// ppg_debug_camera_rays (include/ppg_testhooks.h): camera_ray over the whole film for the samples first .. first + n_samples - 1, as
// { o, mint } { d, maxt } per (sample, pixel)
static __global__ __launch_bounds__(256) void k_debug_camera_rays(DevCamera cam, unsigned long long seed, unsigned int first, unsigned int n_samples, unsigned int n_pix,
                                                                  float4 *rays) {
    const unsigned int pixel = blockIdx.x * blockDim.x + threadIdx.x;
    if (pixel >= n_pix) return;
    for (unsigned int j = 0; j < n_samples; ++j) {
        const unsigned int key = ppg_path_key(seed, pixel, first + j);
        unsigned int dim;
        F3 o, d;
        float mint, maxt;
        camera_ray(cam, key, pixel, o, d, mint, maxt, dim);
        const size_t i = (size_t)j * n_pix + pixel;
        rays[2 * i] = make_float4(o.x, o.y, o.z, mint);
        rays[2 * i + 1] = make_float4(d.x, d.y, d.z, maxt);
    }
}

// grid[cell] for stree_lookup: descend at most PPG_GRID_LEVELS levels along the cell's coordinate bits
static __global__ void k_build_grid(const int4 *stree, unsigned int *grid) {
    unsigned int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= PPG_GRID_DIM * PPG_GRID_DIM * PPG_GRID_DIM) return;
    unsigned int coord[3] = {c % PPG_GRID_DIM, (c / PPG_GRID_DIM) % PPG_GRID_DIM, c / (PPG_GRID_DIM * PPG_GRID_DIM)};
    int used[3] = {0, 0, 0};
    int idx = 0, depth = 0;
    for (; depth < PPG_GRID_LEVELS; ++depth) {
        int4 n = stree[idx];
        if (n.y == 0) break;
        int a = n.x;
        unsigned int bit = (coord[a] >> (PPG_GRID_BITS - 1 - used[a])) & 1u;
        ++used[a];
        idx = bit ? n.z : n.y;
    }
    grid[c] = (unsigned int)idx | ((unsigned int)depth << 27);
}

// copy every workgroup's queue slice into one dense array (offsets = exclusive scan of the slice counts)
static __global__ void k_gather_slices(const unsigned int *items, const unsigned int *count, const unsigned int *offsets, unsigned int cap,
                                unsigned int *dense) {
    const unsigned int b = blockIdx.x, n = count[b], off = offsets[b];
    for (unsigned int k = threadIdx.x; k < n; k += blockDim.x) dense[off + k] = items[(size_t)b * cap + k];
}

// After a bounce: offsets[b] = exclusive scan of the output slice counts (k_gather_slices builds the dense list from them), *total_out =
// the number of live paths, also recorded per bounce for the host (which sizes the next batch's schedule by it).  When fewer than
// `stop_below` paths are left, *stop is set: the wavefront kernels of the bounces that were launched beyond this one return at once and
// the persistent threads (k_tail) take the dense list as it is now.  One workgroup of 1024 threads.
static __global__ __launch_bounds__(1024) void k_scan_counts(const unsigned int *counts, unsigned int *offsets, unsigned int n, unsigned long long *total_out,
                                                      unsigned int *bounce_count, unsigned int *stop, unsigned int stop_below) {
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long carry;
    const bool stopped = stop && *stop;  // (read by every thread before thread 0 may write it)
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    if (stopped) return;
    for (unsigned int start = 0; start < n; start += 1024) {
        unsigned int i = start + threadIdx.x;
        unsigned long long v = i < n ? counts[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (unsigned int off = 1; off < 1024; off <<= 1) {
            unsigned long long t = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) offsets[i] = (unsigned int)(carry + part[threadIdx.x] - v);
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total_out = carry;
        if (bounce_count) *bounce_count = (unsigned int)carry;
        if (stop && carry < (unsigned long long)stop_below) *stop = 1u;
    }
}

// ------------------------------------------------------------------------------------------------
// Per-round application of the sampling-fraction optimiser's records
// ------------------------------------------------------------------------------------------------
// compact[i] += Σ_r rep[i][r]; rep = 0.  Idempotent (a second call adds zeros).
static __global__ void k_fold_replicas(unsigned long long *compact, unsigned long long *rep, unsigned int n_nodes) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    unsigned long long s = 0;
    for (int r = 0; r < PPG_REPLICAS; ++r) {
        unsigned long long v = rep[(size_t)i * PPG_REPLICAS + r];
        if (v) { s += v; rep[(size_t)i * PPG_REPLICAS + r] = 0; }
    }
    if (s) compact[i] += s;
}

// nv[i] = number of vertices path i recorded = the number of positions it owns in the Adam record buffer (fast mode)
// (a path still alive when the tail takes over — `straggler` — reserves the maximum; what it does not use stays a hole)
static __global__ void k_path_nv(PathState P, unsigned int *nv, const unsigned char *straggler, unsigned int max_vertices) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n_paths) nv[i] = (straggler && straggler[i]) ? max_vertices : (P.misc[i].z & FL_NV_MASK) >> FL_NV_SHIFT;
}
// Before k_commit: nv8[i] = how many vertex slots of path i this commit takes (0 for a path still alive when the persistent threads took over:
// it is committed after the tail) — k_commit tests ONE BYTE per (slot, path) work item, and four fifths of the items lie beyond their path's
// last vertex: reading the 16-byte path word for each of them was 30 GB of a 127-pass render.  With interleaved path records also the
// contiguous copy of the per-path word (key, dim, flags, leaf) that the items that do commit read.
static __global__ void k_commit_prepare(PathState P, uint4 *misc_out, unsigned char *nv8, const unsigned char *straggler) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_paths) return;
    const uint4 m = P.misc[i];
    if (misc_out) misc_out[i] = m;
    nv8[i] = (straggler && straggler[i]) ? (unsigned char)0 : (unsigned char)((m.z & FL_NV_MASK) >> FL_NV_SHIFT);
}
// the same for the launch over a LIST of paths (the tail's, after it): nv8[k] belongs to list[k] — the items read it in order
static __global__ void k_commit_prepare_list(PathState P, const unsigned int *list, const unsigned long long *list_n, unsigned char *nv8) {
    const unsigned int n = (unsigned int)*list_n;
    for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
        nv8[k] = (unsigned char)((P.misc[list[k]].z & FL_NV_MASK) >> FL_NV_SHIFT);
}
// flag[list[k]] = 1 for the n = *list_n entries of a dense path list
static __global__ void k_mark_list(const unsigned int *list, const unsigned long long *list_n, unsigned char *flag) {
    const unsigned int n = (unsigned int)*list_n;
    for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) flag[list[k]] = 1;
}
// a[i] = i, *total = n (the dense list of a batch that goes to the persistent threads without a wavefront bounce)
static __global__ void k_iota_total(unsigned int *a, unsigned int n, unsigned long long *total) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) a[i] = i;
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = n;
}
// a[i] = v (PathState::medium of a new batch: the sensor's medium)
static __global__ void k_fill_u32(unsigned int *a, unsigned int n, unsigned int v) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) a[i] = v;
}
static __global__ void k_iota(unsigned int *a, unsigned int n) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = i;
}
// ---- stragglers (ppg_hip.hip "Stragglers") ----
// The vertex slots of the n stragglers, from the batch's slots (path orig[j]) to the compact state's (path j); four lanes per path.
static __global__ void k_extract_vertices(PathState P, PathState Ps, unsigned int n, unsigned int max_vertices) {
    const unsigned int q = threadIdx.x & 3u;
    for (unsigned int j = (blockIdx.x * blockDim.x + threadIdx.x) >> 2; j < n; j += (gridDim.x * blockDim.x) >> 2) {
        const unsigned int i = Ps.orig[j];
        // (the recorded vertices AND the slot behind them: a live path has a bounce pending, whose vertex was half written when it was sampled —
        // direction, throughput, BSDF value — and is completed, and counted, by the next k_shade step)
        unsigned int nv = ((Ps.misc[j].z & FL_NV_MASK) >> FL_NV_SHIFT) + 1u;
        if (nv > max_vertices) nv = max_vertices;
        for (unsigned int v = q; v < nv; v += 4u) {
            const size_t a = (size_t)v * P.n_paths + i, b = (size_t)v * Ps.n_paths + j;
            Ps.v_d[b] = P.v_d[a]; Ps.v_thr[b] = P.v_thr[a]; Ps.v_bsdf[b] = P.v_bsdf[a]; Ps.v_rad[b] = P.v_rad[a];
            if (P.v_o) { Ps.v_o[b] = P.v_o[a]; Ps.v_vox[b] = P.v_vox[a]; }
        }
        if (q == 0 && P.nee_cos) Ps.nee_cos[j] = P.nee_cos[i];
    }
}
static __global__ void k_extract_nee_cos(PathState P, PathState Ps, unsigned int n) {
    for (unsigned int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) Ps.nee_cos[j] = P.nee_cos[Ps.orig[j]];
}
// out[i] = the optimiser's variable of S-tree node i (DevTree::theta_frozen)
static __global__ void k_copy_theta(const LeafHdr *hdr, unsigned int n, float *out) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = hdr[i].theta;
}
// keep[i] = Li of path i of the batch (its film kernel runs after the stragglers have ended, when the batch's own state is gone)
static __global__ void k_copy_li(PathState P, float4 *keep) {
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.n_paths; i += gridDim.x * blockDim.x) keep[i] = P.li[i];
}
// ... and the stragglers' own, once they have ended
static __global__ void k_scatter_li(PathState Ps, unsigned int n, float4 *keep) {
    for (unsigned int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) keep[Ps.orig[j]] = Ps.li[j];
}
// base[perm[r]] = first + r * stride: the record positions of the stragglers' vertices in the round that applies them, in the order of
// their paths (perm = the stragglers sorted by their path's index in its batch)
static __global__ void k_ranked_base(unsigned int *base, const unsigned int *perm, unsigned int n, unsigned int first, unsigned int stride) {
    for (unsigned int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) base[perm[r]] = first + r * stride;
}
static __global__ void k_record_keys(const AdamRec *recs, unsigned long long *keys, unsigned int n) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = recs[i].key;
}
// out[k] = recs[idx[k]] for the first n_valid sorted records (what the round hook hands to the other ranks)
static __global__ void k_gather_records(const AdamRec *recs, const unsigned int *idx, AdamRec *out, unsigned int n) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = recs[idx[i]];
}
// first position whose key is >= bound
D unsigned int adam_lower_bound(const unsigned long long *keys, unsigned int n, unsigned long long bound) {
    unsigned int lo = 0, hi = n;
    while (lo < hi) {
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < bound) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// Sharded optimiser (include/ppg.h): bounds[r] = first record (in key order) of owner r = first key >= (r * segment) << LEAF_SHIFT
static __global__ void k_owner_bounds(const unsigned long long *keys, unsigned int n, unsigned int segment, unsigned int world, unsigned long long *bounds) {
    const unsigned int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > world) return;
    bounds[r] = r == world ? (unsigned long long)adam_lower_bound(keys, n, ~0ull)
                           : (unsigned long long)adam_lower_bound(keys, n, (unsigned long long)((unsigned long long)r * segment) << PPG_ADAM_LEAF_SHIFT);
}
// AdamOptimizer::State of every S-tree node <-> six 32-bit words per node (theta, iter, m, v, batchGradient, batchAccumulation)
template <bool IMPORT>
__global__ void k_adam_state(LeafHdr *hdr, unsigned int n_nodes, unsigned int *state) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    unsigned int *w = state + 6 * (size_t)i;
    LeafHdr &h = hdr[i];
    if (IMPORT) {
        h.theta = __uint_as_float(w[0]); h.adam_iter = (int)w[1]; h.adam_m = __uint_as_float(w[2]); h.adam_v = __uint_as_float(w[3]);
        h.adam_bg = __uint_as_float(w[4]); h.adam_ba = __uint_as_float(w[5]);
    } else {
        w[0] = __float_as_uint(h.theta); w[1] = (unsigned int)h.adam_iter; w[2] = __float_as_uint(h.adam_m); w[3] = __float_as_uint(h.adam_v);
        w[4] = __float_as_uint(h.adam_bg); w[5] = __float_as_uint(h.adam_ba);
    }
}
static __global__ void k_count_valid(const unsigned long long *keys, unsigned int n, unsigned int *out, unsigned long long bound) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = adam_lower_bound(keys, n, bound);
}
// count[k] = records of the optimiser for the k-th S-tree leaf, order[k] = k: sorted by count (descending) they are k_adam_apply's schedule
static __global__ void k_adam_counts(const unsigned int *leaves, unsigned int n_leaves, const unsigned long long *keys, unsigned int n, unsigned int *count, unsigned int *order) {
    const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_leaves) return;
    const unsigned int leaf = leaves[k];
    const unsigned int lo = adam_lower_bound(keys, n, (unsigned long long)leaf << PPG_ADAM_LEAF_SHIFT);
    const unsigned int hi = adam_lower_bound(keys, n, (unsigned long long)(leaf + 1u) << PPG_ADAM_LEAF_SHIFT);
    count[k] = hi - lo; order[k] = k;
}

// The deferred optimizeBsdfSamplingFraction calls of one round (include/ppg.h "Learning the BSDF sampling fraction"): one WAVE
// per S-tree leaf walks that leaf's records in key order — 64 records are fetched at once, then applied in that order with
// the reference's arithmetic: the gradient at the current variable (GP:672-691; every lane its own record, once per batch of append()),
// AdamOptimizer::append (GP:85-95) and step (GP:97-109; the same scalar sequence in every lane).  Lane 0 writes the state back.
static __global__ __launch_bounds__(256) void k_adam_apply(LeafHdr *hdr, const unsigned int *leaves, const unsigned int *order, unsigned int n_leaves,
                                                    const unsigned long long *keys, const unsigned int *idx, const AdamRec *recs, unsigned int n, int loss) {
    const unsigned int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned int lane = threadIdx.x & 63u;
    if (w >= n_leaves) return;
    const unsigned int leaf = leaves[order ? order[w] : w];  // (order: busiest D-trees first, k_adam_counts)
    const unsigned int lo = adam_lower_bound(keys, n, (unsigned long long)leaf << PPG_ADAM_LEAF_SHIFT);
    const unsigned int hi = adam_lower_bound(keys, n, (unsigned long long)(leaf + 1u) << PPG_ADAM_LEAF_SHIFT);
    if (lo == hi) return;
    const LeafHdr h = hdr[leaf];
    float variable = h.theta, firstMoment = h.adam_m, secondMoment = h.adam_v, batchGradient = h.adam_bg, batchAccumulation = h.adam_ba;
    int iter = h.adam_iter;
    // functions of the variable alone, refreshed after every step (the reference re-evaluates them per record: same values)
    float samplingFraction = logistic(variable);
    float dFraction = samplingFraction * (1 - samplingFraction);
    float l2RegGradient = 0.01f * variable;
    for (unsigned int base = lo; base < hi; base += 64u) {
        float4 pay = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float wgt = 0.0f;
        if (base + lane < hi) {
            const AdamRec *r = recs + idx[base + lane];
            const float4 a = reinterpret_cast<const float4 *>(r)[0], b = reinterpret_cast<const float4 *>(r)[1];
            pay = make_float4(a.z, a.w, b.x, b.y);  // product, woPdf, bsdfPdf, dTreePdf
            wgt = b.z;
        }
        const unsigned int cnt = (hi - base) < 64u ? (hi - base) : 64u;
        // Which records complete a batch depends on the weights only (append(), GP:85-95: batchAccumulation += weight; step once it
        // exceeds batchSize = 1) — so the steps' iteration numbers are known before any gradient is: the lanes work out the learning
        // rates of "their" steps (the two pow() of GP:100 are the longest dependency chain of a step) in parallel, off the serial path.
        unsigned long long stepMask = 0ull;
        {
            // (record t is read with v_readlane — t is uniform —, not with a shuffle through the LDS crossbar: the walk over a D-tree's
            // records is a serial chain, and five ds_bpermute round trips per record were most of it)
            float ba = batchAccumulation;
            for (unsigned int t = 0; t < cnt; ++t) {
                ba += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wgt), (int)t));
                if (ba > 1.0f) { stepMask |= 1ull << t; ba = 0; }
            }
        }
        float myLr = 0.0f;
        if ((stepMask >> lane) & 1ull) {
            const int it = iter + (int)__popcll(stepMask & ((2ull << lane) - 1ull));
            myLr = ppg_adam_learning_rate(0.01f, 0.9f, 0.999f, it);  // GP:100, evaluated in double like the reference (ppg_detmath.h)
        }
        for (unsigned int t = 0; t < cnt;) {
            // Every lane: the gradient of ITS record at the current variable (optimizeBsdfSamplingFraction, GP:672-691).  The records up to the
            // next step see the same variable, so one evaluation — two IEEE divisions, the longest links of the chain — serves the whole
            // batch (two records at weight 1, three at the kick-start's 0.5) instead of one evaluation per record; the lanes beyond the
            // batch compute values nobody reads.  Same expressions, same order of the sums: same bits.
            const float mixPdf = samplingFraction * pay.z + (1 - samplingFraction) * pay.w;
            const float r = pay.x / mixPdf;
            const float ratio = (loss == LOSS_KL) ? r : r * r;
            const float dLoss_dSamplingFraction = -ratio / pay.y * (pay.z - pay.w);
            const float dLoss_dVariable = dLoss_dSamplingFraction * dFraction;
            const float lossGradient = l2RegGradient + dLoss_dVariable;
            const float weighted = lossGradient * wgt;
            bool step = false;
            do {  // AdamOptimizer::append, GP:85-95 (batchSize = 1)
                batchGradient += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(weighted), (int)t));
                batchAccumulation += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wgt), (int)t));
                step = batchAccumulation > 1.0f;
                ++t;
            } while (!step && t < cnt);
            if (step) {
                const float gradient = batchGradient / batchAccumulation;  // step(), GP:97-109
                ++iter;
                const float lr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myLr), (int)(t - 1u)));
                firstMoment = 0.9f * firstMoment + (1 - 0.9f) * gradient;
                secondMoment = 0.999f * secondMoment + (1 - 0.999f) * gradient * gradient;
                variable -= lr * firstMoment / (__builtin_sqrtf(secondMoment) + 1e-08f);
                variable = ppg_min(ppg_max(variable, -20.0f), 20.0f);
                batchGradient = 0;
                batchAccumulation = 0;
                samplingFraction = logistic(variable);
                dFraction = samplingFraction * (1 - samplingFraction);
                l2RegGradient = 0.01f * variable;
            }
        }
    }
    if (lane == 0) {
        LeafHdr o = h;
        o.theta = variable; o.adam_iter = iter; o.adam_m = firstMoment; o.adam_v = secondMoment; o.adam_bg = batchGradient; o.adam_ba = batchAccumulation;
        hdr[leaf] = o;
    }
}

// ------------------------------------------------------------------------------------------------
// k_film — block->put / squaredBlock->put / film->put for the spp samples of each owned pixel
// (GP:1633-1640; box filter ⇒ own pixel, unit weight)
// ------------------------------------------------------------------------------------------------
static __global__ void k_film(PathState P, int spp, float *image, float *sq_image, float *image_w, float *film, float *film_w) {
    unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.n_pix) return;
    unsigned int pixel = P.pixels[k];
    float ir = image[3 * pixel], ig = image[3 * pixel + 1], ib = image[3 * pixel + 2];
    float sr = sq_image[3 * pixel], sg = sq_image[3 * pixel + 1], sb = sq_image[3 * pixel + 2];
    float fr = film[3 * pixel], fg = film[3 * pixel + 1], fb = film[3 * pixel + 2];
    float iw = image_w[pixel], fw = film_w[pixel];
    for (int j = 0; j < spp; ++j) {
        float4 l = P.li[(size_t)j * P.n_pix + k];
        ir += l.x; ig += l.y; ib += l.z;
        sr += l.x * l.x; sg += l.y * l.y; sb += l.z * l.z;
        fr += l.x; fg += l.y; fb += l.z;
        iw += 1.0f; fw += 1.0f;
    }
    image[3 * pixel] = ir; image[3 * pixel + 1] = ig; image[3 * pixel + 2] = ib;
    sq_image[3 * pixel] = sr; sq_image[3 * pixel + 1] = sg; sq_image[3 * pixel + 2] = sb;
    film[3 * pixel] = fr; film[3 * pixel + 1] = fg; film[3 * pixel + 2] = fb;
    image_w[pixel] = iw; film_w[pixel] = fw;
}

// The same for the passes of a FINAL iteration (include/ppg.h "Final iteration: groups of passes"): the samples of a pixel are summed per GROUP
// of passes, in sample order and from whatever the group's partial holds (zero, or an earlier launch's part of the same group), into the
// group's slot of `partials` — one slot = image (3 n), squared image (3 n), weights (n), n = pixels of the whole film.  k_add_groups then adds
// the slots to image / squared image / weights / film in group order.  On one GPU that is the same sum as k_film's up to the association of
// the float additions; it is what lets the groups of a sharded render be rendered whole by different ranks and still add up to the same bits.
static __global__ void k_film_groups(PathState P, int spp, unsigned int group_samples, float *partials, unsigned int slot0, unsigned int slot_stride, unsigned int n_img) {
    unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.n_pix) return;
    const unsigned int pixel = P.pixels[k];
    for (int j0 = 0; j0 < spp; j0 += (int)group_samples) {
        float *slot = partials + (size_t)(slot0 + (unsigned int)(j0 / (int)group_samples) * slot_stride) * 7u * n_img;
        float *im = slot + 3 * (size_t)pixel, *sq = slot + 3 * (size_t)n_img + 3 * (size_t)pixel, *w = slot + 6 * (size_t)n_img + pixel;
        float ir = im[0], ig = im[1], ib = im[2], sr = sq[0], sg = sq[1], sb = sq[2], iw = *w;
        const int j1 = j0 + (int)group_samples < spp ? j0 + (int)group_samples : spp;
        for (int j = j0; j < j1; ++j) {
            const float4 l = P.li[(size_t)j * P.n_pix + k];
            ir += l.x; ig += l.y; ib += l.z;
            sr += l.x * l.x; sg += l.y * l.y; sb += l.z * l.z;
            iw += 1.0f;
        }
        im[0] = ir; im[1] = ig; im[2] = ib; sq[0] = sr; sq[1] = sg; sq[2] = sb; *w = iw;
    }
}
// image += slot, squared image += slot, weights += slot, film += slot (image part), film weights += slot, for slots first .. first + count - 1
// in this order; the slots are zeroed.
static __global__ void k_add_groups(unsigned int n_img, float *partials, unsigned int first, unsigned int count, float *image, float *sq_image, float *image_w,
                                    float *film, float *film_w) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    float im[3] = {image[3 * i], image[3 * i + 1], image[3 * i + 2]}, sq[3] = {sq_image[3 * i], sq_image[3 * i + 1], sq_image[3 * i + 2]};
    float fi[3] = {film[3 * i], film[3 * i + 1], film[3 * i + 2]}, iw = image_w[i], fw = film_w[i];
    for (unsigned int g = first; g < first + count; ++g) {
        float *slot = partials + (size_t)g * 7u * n_img;
        for (int c = 0; c < 3; ++c) {
            const float a = slot[3 * (size_t)i + c], b = slot[3 * (size_t)n_img + 3 * (size_t)i + c];
            im[c] += a; sq[c] += b; fi[c] += a;
            slot[3 * (size_t)i + c] = 0.0f; slot[3 * (size_t)n_img + 3 * (size_t)i + c] = 0.0f;
        }
        const float w = slot[6 * (size_t)n_img + i];
        iw += w; fw += w;
        slot[6 * (size_t)n_img + i] = 0.0f;
    }
    for (int c = 0; c < 3; ++c) { image[3 * i + c] = im[c]; sq_image[3 * i + c] = sq[c]; film[3 * i + c] = fi[c]; }
    image_w[i] = iw; film_w[i] = fw;
}

// ------------------------------------------------------------------------------------------------
// Reconstruction filters other than the default box (include/ppg.h ppg_set_rfilter): ImageBlock::put (imageblock.h:147-190) with the
// discretised table of ReconstructionFilter::configure (rfilter.cpp:37-55), made deterministic through FOOTPRINT partials.
//   F = float[taps][7][W * H], taps = (2B + 1)², tap o = (dy + B) * (2B + 1) + (dx + B); the slot (o, c) that source pixel s adds to target
//   pixel s + (dx, dy) lives at F[(o * 7 + c) * W * H + s] — indexed by the SOURCE pixel, so the 64 lanes of a wave (neighbouring source
//   pixels of a row) read and write 64 consecutive floats per (o, c), and the resolve's lanes (neighbouring targets) read 64 consecutive
//   floats too (DESIGN.md "Film reconstruction filter").  c = image RGB, squared image RGB, weight.
// ------------------------------------------------------------------------------------------------
// (FilmFilter: ppg_kernels.h, which the feature-buffer kernels share it through)

// Source pixel P.pixels[k] (one thread each) adds the launch's samples [j0, j1) — w·L, w·L², w per tap, in sample order — to its footprint
// slots.  The sample position is recomputed from the path key exactly as k_generate draws it (same sample index formula, dims 0 and 1).
// Taps are walked row by row: one row's (2B + 1) x 7 accumulators stay in registers while the samples go by.
template <int B>
__global__ __launch_bounds__(256) void k_film_filter(PathState P, FilmFilter ff, unsigned long long seed, unsigned int pass_index_spp,
                                                     unsigned int group_samples, unsigned int group_stride, int j0, int j1, float *foot) {
    constexpr int T = 2 * B + 1;
    __shared__ float tab[32];
    if (threadIdx.x < 32) tab[threadIdx.x] = ff.table[threadIdx.x];
    __syncthreads();
    const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P.n_pix) return;
    const unsigned int pixel = P.pixels[k];
    const int W = ff.W, H = ff.H;
    const size_t n = (size_t)W * (size_t)H;
    const int px = (int)(pixel % (unsigned int)W), py = (int)(pixel / (unsigned int)W);
    const float r = ff.radius, scale = ff.scale;
    for (int dy = -B; dy <= B; ++dy) {
        const int ty = py + dy;
        if (ty < 0 || ty >= H) continue;
        float acc[T][7];
#pragma unroll
        for (int dx = -B; dx <= B; ++dx) {
            const int tx = px + dx;
            const size_t o = (size_t)((dy + B) * T + (dx + B));
#pragma unroll
            for (int c = 0; c < 7; ++c) acc[dx + B][c] = (tx >= 0 && tx < W) ? foot[(o * 7 + c) * n + pixel] : 0.0f;
        }
        for (int j = j0; j < j1; ++j) {
            const unsigned int ju = (unsigned int)j;
            const unsigned int sample = group_samples ? pass_index_spp + (ju / group_samples) * group_stride + (ju % group_samples) : pass_index_spp + ju;
            const unsigned int key = ppg_path_key(seed, pixel, sample);
            const float u1 = ppg_rand(key, 0u), u2 = ppg_rand(key, 1u);
            const float posx = ((float)px + u1) - 0.5f, posy = ((float)py + u2) - 0.5f;  // samplePos (GP:1620) - 0.5
            const int ylo = max((int)ceilf(posy - r), 0), yhi = min((int)floorf(posy + r), H - 1);
            if (ty < ylo || ty > yhi) continue;
            const int xlo = max((int)ceilf(posx - r), 0), xhi = min((int)floorf(posx + r), W - 1);
            const float wy = tab[min((int)fabsf(((float)ty - posy) * scale), 31)];
            const float4 l = P.li[(size_t)j * P.n_pix + k];
            const float qx = l.x * l.x, qy = l.y * l.y, qz = l.z * l.z;  // spec * spec, put into the squared block
#pragma unroll
            for (int dx = -B; dx <= B; ++dx) {
                const int tx = px + dx;
                if (tx < xlo || tx > xhi) continue;
                const float w = tab[min((int)fabsf(((float)tx - posx) * scale), 31)] * wy;
                acc[dx + B][0] += w * l.x; acc[dx + B][1] += w * l.y; acc[dx + B][2] += w * l.z;
                acc[dx + B][3] += w * qx; acc[dx + B][4] += w * qy; acc[dx + B][5] += w * qz;
                acc[dx + B][6] += w;
            }
        }
#pragma unroll
        for (int dx = -B; dx <= B; ++dx) {
            const int tx = px + dx;
            if (tx < 0 || tx >= W) continue;
            const size_t o = (size_t)((dy + B) * T + (dx + B));
#pragma unroll
            for (int c = 0; c < 7; ++c) foot[(o * 7 + c) * n + pixel] = acc[dx + B][c];
        }
    }
}

// Target pixel t (one thread each, the whole film) sums its taps from zero — dy = -B .. B, within each dy dx = -B .. B; the tap (dx, dy)
// holds what source pixel t - (dx, dy) put there — zeroes them, and adds the sums to im (3 n) / sq (3 n) / w (n) and, if film != nullptr, to
// film / film_w: the image of a ppg_render_passes() call and the iteration's film, or (film == nullptr) a final group's partial slot.
template <int B>
__global__ __launch_bounds__(256) void k_film_resolve(FilmFilter ff, float *foot, float *im, float *sq, float *w, float *film, float *film_w) {
    constexpr int T = 2 * B + 1;
    const int W = ff.W, H = ff.H;
    const size_t n = (size_t)W * (size_t)H;
    const unsigned int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int tx = (int)(t % (unsigned int)W), ty = (int)(t / (unsigned int)W);
    float s[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = -B; dy <= B; ++dy) {
        const int sy = ty - dy;
        if (sy < 0 || sy >= H) continue;
#pragma unroll
        for (int dx = -B; dx <= B; ++dx) {
            const int sx = tx - dx;
            if (sx < 0 || sx >= W) continue;
            const size_t o = (size_t)((dy + B) * T + (dx + B)), src = (size_t)sy * W + sx;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                float *f = foot + (o * 7 + c) * n + src;
                s[c] += *f;
                *f = 0.0f;
            }
        }
    }
    for (int c = 0; c < 3; ++c) { im[3 * (size_t)t + c] += s[c]; sq[3 * (size_t)t + c] += s[3 + c]; }
    w[t] += s[6];
    if (film) {
        for (int c = 0; c < 3; ++c) film[3 * (size_t)t + c] += s[c];
        film_w[t] += s[6];
    }
}

// ------------------------------------------------------------------------------------------------
// A filtered film sharded by tiles (include/ppg.h "Footprint hook").  A BORDER SLOT is a (source pixel s, tap o) whose target s + (dx, dy)
// lies inside the film on a tile of ANOTHER rank than s's; the M border slots are numbered tap by tap (o ascending) and, within a tap, by
// source pixel (row-major) — the same numbering on every rank.  slot_src[m] = s, slot_tap[m] = o.  The halo buffer is channel-major,
// halo[c * M + m], c = 0 .. 6: the lanes of a wave take consecutive slots — neighbouring source pixels of one tap — and so read and write
// consecutive floats of the footprint (source-major) and of the halo alike.
//   k_halo_pack    list = the slots whose SOURCE this rank owns: footprint → halo, and the footprint slot is zeroed.  The rest of the halo
//                  was zeroed beforehand, so every float of it is non-zero on one rank at most and the all-reduce (sum) is exact.
//   k_halo_unpack  list = the slots whose TARGET this rank owns: halo (after the exchange) → footprint, at the foreign source's position,
//                  which no kernel of this rank wrote.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_halo_pack(const unsigned int *list, unsigned int count, const unsigned int *slot_src, const unsigned char *slot_tap,
                                                   unsigned int M, size_t n, float *foot, float *halo) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned int m = list[i];
    float *f = foot + (size_t)slot_tap[m] * 7 * n + slot_src[m];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        halo[(size_t)c * M + m] = f[(size_t)c * n];
        f[(size_t)c * n] = 0.0f;
    }
}
static __global__ __launch_bounds__(256) void k_halo_unpack(const unsigned int *list, unsigned int count, const unsigned int *slot_src, const unsigned char *slot_tap,
                                                     unsigned int M, size_t n, float *foot, const float *halo) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned int m = list[i];
    float *f = foot + (size_t)slot_tap[m] * 7 * n + slot_src[m];
#pragma unroll
    for (int c = 0; c < 7; ++c) f[(size_t)c * n] = halo[(size_t)c * M + m];
}
// k_film_resolve for the targets this rank owns only (pixels = its owned-pixel list, row-major inside its tiles): the same taps in the same
// order from zero, so a pixel's sums are the unsharded resolve's bit for bit once the foreign slots have been unpacked; every other pixel of
// im / sq / w / film / film_w stays untouched (the image and film exchanges keep their disjoint supports).  The slots read are zeroed; those
// of own sources towards foreign targets were zeroed by k_halo_pack, and nothing else was ever written: the whole footprint is zero again.
template <int B>
__global__ __launch_bounds__(256) void k_film_resolve_owned(FilmFilter ff, const unsigned int *pixels, unsigned int n_own, float *foot, float *im, float *sq, float *w,
                                                            float *film, float *film_w) {
    constexpr int T = 2 * B + 1;
    const int W = ff.W, H = ff.H;
    const size_t n = (size_t)W * (size_t)H;
    const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_own) return;
    const unsigned int t = pixels[k];
    const int tx = (int)(t % (unsigned int)W), ty = (int)(t / (unsigned int)W);
    float s[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = -B; dy <= B; ++dy) {
        const int sy = ty - dy;
        if (sy < 0 || sy >= H) continue;
#pragma unroll
        for (int dx = -B; dx <= B; ++dx) {
            const int sx = tx - dx;
            if (sx < 0 || sx >= W) continue;
            const size_t o = (size_t)((dy + B) * T + (dx + B)), src = (size_t)sy * W + sx;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                float *f = foot + (o * 7 + c) * n + src;
                s[c] += *f;
                *f = 0.0f;
            }
        }
    }
    for (int c = 0; c < 3; ++c) { im[3 * (size_t)t + c] += s[c]; sq[3 * (size_t)t + c] += s[3 + c]; }
    w[t] += s[6];
    if (film) {
        for (int c = 0; c < 3; ++c) film[3 * (size_t)t + c] += s[c];
        film_w[t] += s[6];
    }
}

// per-pixel variance estimate of performRenderPasses (GP:1300-1311); the clamped luminance goes to `lum`, stored x-major
// (index x * H + y) — the order the reference's serial loop sums it in, so the host adds a contiguous array
static __global__ void k_variance(int n, int W, int N, const float *image, const float *sq_image, const float *image_w, float *var_rgb, float *lum) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float w = image_w[i];
    float iw = w != 0 ? 1.0f / w : 0.0f;
    F3 pixel = f3(image[3 * i] * iw, image[3 * i + 1] * iw, image[3 * i + 2] * iw);
    F3 sq = f3(sq_image[3 * i] * iw, sq_image[3 * i + 1] * iw, sq_image[3 * i + 2] * iw);
    F3 localVar = sq - div3(mul3(pixel, pixel), (float)N);
    var_rgb[3 * i] = localVar.x; var_rgb[3 * i + 1] = localVar.y; var_rgb[3 * i + 2] = localVar.z;
    float l = localVar.x * 0.212671f + localVar.y * 0.715160f + localVar.z * 0.072169f;
    const int x = i % W, y = i / W, H = n / W;
    lum[(size_t)x * H + y] = ppg_min(l, 10000.0f);
}

static __global__ void k_normalise(int n, const float *rgb_sum, const float *w, float *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float ww = w[i];
    float iw = ww != 0 ? 1.0f / ww : 0.0f;
    out[3 * i] = rgb_sum[3 * i] * iw; out[3 * i + 1] = rgb_sum[3 * i + 1] * iw; out[3 * i + 2] = rgb_sum[3 * i + 2] * iw;
}

static __global__ void k_axpy(int n, float a, const float *x, float *y) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += x[i] * a;
}

// ------------------------------------------------------------------------------------------------
// SD-tree rebuild kernels
// ------------------------------------------------------------------------------------------------
// DTree::reset (GP:456-514): one lane walks the reference's LIFO stack for one S-tree leaf, so the node
// numbering equals the reference's.  WRITE = false only counts nodes (first pass); an exclusive scan over
// the counts gives every leaf its block in the building pool; WRITE = true emits the child indices.
template <bool WRITE>
__global__ void k_dtree_reset(DevTree T, const unsigned int *leaves, unsigned int n_leaves, int newMaxDepth, float rho,
                              unsigned int *counts, ushort4 *bchild_out) {
    unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_leaves) return;
    const unsigned int leaf = leaves[k];
    const LeafHdr h = T.hdr[leaf];
    const float total = h.s_sum;
    const SNode *prev = T.snodes + h.s_base;
    const unsigned int base = WRITE ? h.b_base : 0;
    struct E { unsigned short nodeIndex, otherIndex; unsigned char depth, isThis; float val; };
    E st[64];
    int sp = 0;
    st[sp++] = E{0, 0, 1, 0, 0.0f};
    unsigned int size = 1;
    int maxDepth = 0;
    if (WRITE) bchild_out[base] = make_ushort4(0, 0, 0, 0);
    bool abort = false;
    while (sp && !abort) {
        E s = st[--sp];
        if ((int)s.depth > maxDepth) maxDepth = s.depth;
        unsigned short ch[4] = {0, 0, 0, 0};
        SNode other;
        if (!s.isThis) other = prev[s.otherIndex];
        for (int i = 0; i < 4; ++i) {
            const float osum = s.isThis ? s.val : other.sum[i];
            const float fraction = total > 0 ? (osum / total) : ppg_exp2i(-2 * (int)s.depth);
            if ((int)s.depth < newMaxDepth && fraction > rho) {
                if (!s.isThis && other.child[i] != 0) st[sp++] = E{(unsigned short)size, other.child[i], (unsigned char)(s.depth + 1), 0, 0.0f};
                else st[sp++] = E{(unsigned short)size, (unsigned short)size, (unsigned char)(s.depth + 1), 1, osum / 4};
                ch[i] = (unsigned short)size;
                if (WRITE) bchild_out[base + size] = make_ushort4(0, 0, 0, 0);
                ++size;
                if (size > 65535u) { abort = true; break; }
            }
        }
        if (WRITE) bchild_out[base + s.nodeIndex] = make_ushort4(ch[0], ch[1], ch[2], ch[3]);
    }
    if (!WRITE) counts[k] = size;
    else { T.hdr[leaf].b_depth = maxDepth; }
}

// DTree::build (GP:520-533, 346-366) + `sampling = building` (GP:610-613): children always have larger
// indices than their parent, so one backwards sweep evaluates the recursion's post-order.
static __global__ void k_dtree_build(DevTree T, const unsigned int *leaves, unsigned int n_leaves, SNode *snodes_out) {
    unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_leaves) return;
    const unsigned int leaf = leaves[k];
    LeafHdr h = T.hdr[leaf];
    const unsigned int base = h.b_base;
    for (int n = (int)h.b_num - 1; n >= 0; --n) {
        ushort4 c4 = T.bchild[base + n];
        const unsigned short cc[4] = {c4.x, c4.y, c4.z, c4.w};
        SNode out;
        for (int j = 0; j < 4; ++j) {
            out.child[j] = cc[j];
            if (cc[j] == 0) {
                out.sum[j] = ppg_from_fixed(T.bacc[(size_t)(base + n) * 4 + j]);
            } else {
                const SNode c = snodes_out[base + cc[j]];
                float sum = 0;
                for (int q = 0; q < 4; ++q) sum += c.sum[q];
                out.sum[j] = sum;
            }
        }
        out.pad[0] = out.pad[1] = 0;
        snodes_out[base + n] = out;
    }
    const SNode root = snodes_out[base];
    float sum = 0;
    for (int i = 0; i < 4; ++i) sum += root.sum[i];
    h.s_base = base; h.s_num = h.b_num; h.s_depth = h.b_depth;
    h.s_sum = sum;
    h.s_statw = ppg_from_fixed(T.bweight[leaf]);
    h.b_statw = h.s_statw;
    T.hdr[leaf] = h;
}

// ------------------------------------------------------------------------------------------------
// STree::refine (GP:957-998) + STreeNode::subdivide (GP:876-895) on the device
// ------------------------------------------------------------------------------------------------
// The reference walks the tree with an explicit LIFO stack (child 0 pushed first, so child 1 is visited first) and
// subdivides a leaf while its building weight exceeds the threshold; every subdivision appends two nodes that inherit the
// parent's D-trees with half its weight.  A leaf of weight W therefore becomes a COMPLETE binary subtree of depth
// n = #{halvings until W / 2^n <= threshold}, all of whose 2^n - 1 subdivisions happen consecutively (the stack finishes a
// subtree before anything else), in right-first preorder.  With the old leaves kept in that right-first order (`dfs`), node
// numbers are closed-form:
//   first new node of old leaf j      = n_old + 2 * (number of subdivisions of the leaves before j)      (exclusive scan)
//   children of subdivision e of leaf j = base_j + 2 e, base_j + 2 e + 1                                   (e = preorder index)
// so every subdivision of every leaf can be written independently.  Results are identical to the serial loop, node for node.
static __global__ void k_refine_count(const LeafHdr *hdr, const unsigned int *dfs, unsigned int n_leaves, float threshold, unsigned int *events,
                               unsigned int *new_leaves) {
    unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    float w = hdr[dfs[j]].b_statw;
    unsigned int n = 0;
    while (w > threshold && n < 30u) { w = w / 2; ++n; }  // shallSplit (GP:953-955); children get half the weight (GP:886)
    events[j] = (1u << n) - 1u;
    new_leaves[j] = 1u << n;
}

// one workgroup per old leaf; thread e handles subdivision e of that leaf's subtree
static __global__ void k_refine_fill(int4 *stree, LeafHdr *hdr, const unsigned int *dfs, unsigned int n_leaves, unsigned int n_old,
                              const unsigned int *events, const unsigned int *ev_off, const unsigned int *lv_off, unsigned int *dfs_out) {
    const unsigned int j = blockIdx.x;
    if (j >= n_leaves) return;
    const unsigned int L = dfs[j];
    const unsigned int n_ev = events[j];
    if (n_ev == 0) {
        if (threadIdx.x == 0) dfs_out[lv_off[j]] = L;
        return;
    }
    unsigned int n = 0;
    while (((1u << n) - 1u) < n_ev) ++n;  // depth of the complete subtree
    __shared__ LeafHdr H;
    __shared__ int axis0;
    if (threadIdx.x == 0) { H = hdr[L]; axis0 = stree[L].x; }
    __syncthreads();
    const unsigned int base = n_old + 2u * ev_off[j];
    LeafHdr cleared;  // cur.dTree = {} (GP:893)
    {
        unsigned int *z = reinterpret_cast<unsigned int *>(&cleared);
        for (unsigned int q = 0; q < sizeof(LeafHdr) / 4; ++q) z[q] = 0u;
    }
    for (unsigned int e = threadIdx.x; e < n_ev; e += blockDim.x) {
        // locate subdivision e: walk down from the leaf; at depth k each child subtree holds S = 2^(n-k-1) - 1 subdivisions,
        // the right child's come first
        unsigned int node = L, k = 0, cur = 0, rem = e, pos = 0;
        while (rem != 0) {
            rem -= 1;
            const unsigned int S = (1u << (n - k - 1)) - 1u;
            if (rem < S) { node = base + 2u * cur + 1u; cur = cur + 1u; }
            else { rem -= S; node = base + 2u * cur; cur = cur + 1u + S; pos += 1u << (n - k - 1); }
            ++k;
        }
        const unsigned int c0 = base + 2u * e, c1 = c0 + 1u;
        stree[node] = make_int4((axis0 + (int)k) % 3, (int)c0, (int)c1, 0);
        hdr[node] = cleared;
        if (k + 1 == n) {  // the children are the new leaves: copies of the old leaf with the weight halved once per level
            LeafHdr h = H;
            float w = h.b_statw;
            for (unsigned int t = 0; t <= k; ++t) w = w / 2;
            h.b_statw = w;
            const int ax = (axis0 + (int)k + 1) % 3;
            stree[c0] = make_int4(ax, 0, 0, 0); hdr[c0] = h;
            stree[c1] = make_int4(ax, 0, 0, 0); hdr[c1] = h;
            dfs_out[lv_off[j] + pos] = c1;       // right child first
            dfs_out[lv_off[j] + pos + 1u] = c0;
        }
    }
}

// exclusive scan of `counts` (n small: one S-tree leaf each) by a single workgroup; total → *total_out
static __global__ void k_scan_exclusive(const unsigned int *counts, unsigned int *offsets, unsigned int n, unsigned long long *total_out) {
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (unsigned int start = 0; start < n; start += 1024) {
        unsigned int i = start + threadIdx.x;
        unsigned long long v = i < n ? counts[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (unsigned int off = 1; off < 1024; off <<= 1) {
            unsigned long long t = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) offsets[i] = (unsigned int)(carry + part[threadIdx.x] - v);
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

static __global__ void k_assign_blocks(DevTree T, const unsigned int *leaves, unsigned int n_leaves, const unsigned int *counts,
                                const unsigned int *offsets) {
    unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_leaves) return;
    T.hdr[leaves[k]].b_base = offsets[k];
    T.hdr[leaves[k]].b_num = counts[k];
}

// batched queries (ppg_query_pdf / ppg_query_sample)
static __global__ void k_query_pdf(DevTree T, unsigned int n, const float *pos, const float *dirs, float *out) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 vox;
    int leaf = stree_lookup(T, f3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), vox);
    float cx, cy;
    dir_to_canonical(f3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), cx, cy);
    RegColumn col;
    out[i] = dtree_pdf<RegColumn &>(T, dtree_ref(T.hdr[leaf]), cx, cy, col);
}
static __global__ void k_query_sample(DevTree T, unsigned int n, const float *pos, unsigned long long seed, float *out) {
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 vox;
    int leaf = stree_lookup(T, f3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), vox);
    unsigned int key = ppg_path_key(seed, i, 0), dim = 0;
    float cx, cy;
    dtree_sample(T, dtree_ref(T.hdr[leaf]), key, dim, cx, cy);
    F3 d = canonical_to_dir(cx, cy);
    out[3 * i] = d.x; out[3 * i + 1] = d.y; out[3 * i + 2] = d.z;
}

// ppg_debug_commit (include/ppg_testhooks.h): the paths and vertex slots of a PathState from explicit arrays, as k_shade leaves them — the
// per-path word (key, dim, nV), per vertex the leaf and voxel size of stree_lookup at p.  first[i]: path i's first vertex in the arrays.
struct DebugCommitArrays {
    const unsigned int *nv, *key, *dim, *first;
    const float *p, *d, *radiance, *throughput, *bsdf_val, *wo_pdf, *bsdf_pdf, *dtree_pdf;
    const unsigned char *is_delta;
};
static __global__ void k_debug_commit_fill(PathState P, DevTree T, DebugCommitArrays A, unsigned int slots) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_paths) return;
    unsigned int nv = A.nv[i];
    if (nv > slots) nv = slots;  // (the host checked it)
    P.misc[i] = make_uint4(A.key[i], A.dim[i], nv << FL_NV_SHIFT, 0u);
    for (unsigned int v = 0; v < nv; ++v) {
        const size_t g = (size_t)A.first[i] + v, vi = (size_t)v * P.n_paths + i;
        F3 vox;
        const F3 p = f3(A.p[3 * g], A.p[3 * g + 1], A.p[3 * g + 2]);
        const int leaf = stree_lookup(T, p, vox);
        P.v_d[vi] = make_float4(A.d[3 * g], A.d[3 * g + 1], A.d[3 * g + 2], A.wo_pdf[g]);
        P.v_thr[vi] = make_float4(A.throughput[3 * g], A.throughput[3 * g + 1], A.throughput[3 * g + 2], A.bsdf_pdf[g]);
        P.v_bsdf[vi] = make_float4(A.bsdf_val[3 * g], A.bsdf_val[3 * g + 1], A.bsdf_val[3 * g + 2], A.dtree_pdf[g]);
        P.v_rad[vi] = make_float4(A.radiance[3 * g], A.radiance[3 * g + 1], A.radiance[3 * g + 2],
                                  __uint_as_float((unsigned int)leaf | (A.is_delta[g] ? 0x80000000u : 0u)));
        if (P.v_o) {
            P.v_o[vi] = make_float4(p.x, p.y, p.z, 0.0f);
            P.v_vox[vi] = make_float4(vox.x, vox.y, vox.z, 0.0f);
        }
    }
}

#endif
