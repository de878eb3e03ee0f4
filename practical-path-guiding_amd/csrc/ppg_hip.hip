/*
 * ppg_hip.hip — libppg_hip.so: host side of the MI355X guided path tracer behind the C-ABI of include/ppg.h.
 *
 * Host responsibilities (thin): property parsing (GP:1014-1085), BVH build, pool management, the
 * iteration schedule of render()/renderSPP()/renderTime() (GP:1342-1585), the statistics log.  Everything per
 * path, per S-tree / D-tree node or per pixel runs in the kernels of ppg_kernels.h — including the SD-tree rebuild
 * between iterations (S-tree refine, D-tree reset and build); the host keeps a read-back mirror of the S-tree for
 * the log, the dumps and the readers.
 */
#include <hip/hip_runtime.h>

#include <cstring>  // rocprim's texture iterator calls memset from host code
#include <map>
#include <mutex>
#include <set>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ppg.h"
#include "../../include/ppg_mathcheck.h"
#include "../../include/ppg_testhooks.h"
#include "ppg_batch_plan.h"
#include "ppg_host_kernels.h"
#include "ppg_launch.h"
#include "ppg_scene_build.h"
#include "ppg_sdt_load.h"

using namespace ppg_plan;
static_assert(kSpatialFilterBox == SF_BOX && kNeeKickstart == NEE_KICKSTART && kBlock == PPG_BLOCK && kDenseChunk == PPG_DCHUNK && kAdamLeafShift == PPG_ADAM_LEAF_SHIFT,
              "ppg_batch_plan.h restates these values");
static_assert(ppg_sdt::kOk == PPG_OK && ppg_sdt::kErrInvalid == PPG_ERR_INVALID && ppg_sdt::kErrNoMem == PPG_ERR_NOMEM && ppg_sdt::kSpatialFilterBox == SF_BOX &&
                  ppg_sdt::kStreeMaxDepth == PPG_STREE_MAX_DEPTH && ppg_sdt::kPi == PPG_PI_F && sizeof(ppg_sdt::Node) == ppg_sdt::kNodeBytes,
              "ppg_sdt_load.h restates these values");

namespace {

thread_local std::string g_createError;

#define HIP_CHECK(expr)                                                                             \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            ctx->error = std::string(#expr) + ": " + hipGetErrorString(_e);                         \
            return PPG_ERR_DEVICE;                                                                  \
        }                                                                                           \
    } while (0)

// Device memory blocks outlive the contexts that used them: a context's buffers grow while it renders (path state at begin_render, the
// optimiser's records with the first large round, sort scratch ...), and hipMalloc / hipFree of hundreds of megabytes are synchronous,
// millisecond-scale calls — rocprofv3 showed a 17 ms hole in a 190 ms KITCHEN render where one round's record buffers were grown.  Released
// blocks therefore go to a process-wide cache (per device, keyed by size) and the next reserve() — of this context or of the next one, e.g.
// the render after a warm-up render — takes a fitting block from it.  Blocks come back with stale contents, like fresh hipMalloc memory.
// Ordering: a block is released only by reserve() / the destructor on the host; everything that used it was enqueued earlier on the
// context's in-order stream (the second stream is joined back before the host continues past a batch), and its next user is enqueued later.
// The stream the calling thread's context works on (set by the C-ABI entry points that render): fresh blocks are touched on it and the
// hand-over of a released block is ordered behind it — not behind the legacy null stream, which would serialise every stream of the
// process.  Outside those entry points (scene set-up, destruction) it is null and the null stream's conservative ordering applies.
thread_local hipStream_t g_ctxStream = nullptr;
struct StreamScope {
    hipStream_t prev;
    explicit StreamScope(hipStream_t s) : prev(g_ctxStream) { g_ctxStream = s; }
    ~StreamScope() { g_ctxStream = prev; }
};

struct BlockCache {
    struct Block { void *p; hipEvent_t ready; };  // `ready`: recorded when the block was released, behind everything its last owner had enqueued
    std::mutex m;
    std::map<int, std::multimap<size_t, Block>> blocks;
    size_t held = 0;
    size_t maxHeld = 0;  // a third of the device's memory (set on first use): the cache must not starve other processes of the GPU
    static constexpr size_t kGranule = (size_t)2 << 20;
    static size_t roundUp(size_t bytes) { return (bytes + kGranule - 1) / kGranule * kGranule; }
    void *take(size_t bytes, size_t &got) {
        int dev = 0; (void)hipGetDevice(&dev);
        Block b{nullptr, nullptr};
        {
            std::lock_guard<std::mutex> g(m);
            auto &mm = blocks[dev];
            auto it = mm.lower_bound(bytes);
            if (it == mm.end() || it->first > std::max(2 * bytes, bytes + ((size_t)64 << 20))) return nullptr;
            b = it->second; got = it->first;
            held -= got; mm.erase(it);
        }
        // the previous owner may be another context on another stream: its work on the block must be over before the new owner touches it
        if (b.ready) { (void)hipEventSynchronize(b.ready); (void)hipEventDestroy(b.ready); }
        return b.p;
    }
    void give(void *p, size_t bytes) {
        int dev = 0; (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(m);
            if (!maxHeld) { size_t fr = 0, tot = 0; maxHeld = hipMemGetInfo(&fr, &tot) == hipSuccess ? tot / 3 : ((size_t)32 << 30); }
            static const bool debugAlloc = getenv("PPG_DEBUG_ALLOC") != nullptr;
            if (debugAlloc && held + bytes > maxHeld) fprintf(stderr, "[ppg alloc] hipFree %zu MiB (cache full: %zu MiB)\n", bytes >> 20, held >> 20);
            if (held + bytes <= maxHeld) {
                Block b{p, nullptr};
                if (hipEventCreateWithFlags(&b.ready, hipEventDisableTiming) == hipSuccess) (void)hipEventRecord(b.ready, g_ctxStream);
                else b.ready = nullptr;
                if (!b.ready) (void)hipDeviceSynchronize();
                blocks[dev].emplace(bytes, b); held += bytes;
                return;
            }
        }
        (void)hipFree(p);
    }
    // Before a context's streams are destroyed: the `ready` events of cached blocks may have been recorded on them, and the runtime
    // dereferences an event's stream when the event is waited for (seen as a spurious "operation not permitted when stream is
    // capturing" from hipEventSynchronize after the stream was gone).  The streams have been synchronised: the events are complete.
    void settle() {
        int dev = 0; (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> g(m);
        for (auto &kv : blocks[dev])
            if (kv.second.ready) { (void)hipEventSynchronize(kv.second.ready); (void)hipEventDestroy(kv.second.ready); kv.second.ready = nullptr; }
    }
    // Scene set-up: spare blocks for what a render grows as it goes — the SD-tree's pools, the per-iteration images, the straggler sets' small
    // arrays: dozens of allocations of 2 - 30 MB whose sizes depend on the scene.  Each is a synchronous hipMalloc of 0.1 - 0.2 ms when the cache
    // is empty, i.e. in the FIRST render of a process (5 % of a 20-pass KITCHEN render); with spares in the cache they are not.  Once per device.
    void prewarm() {
        int dev = 0; (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(m);
            if (warmed.count(dev)) return;
            warmed.insert(dev);
        }
        static const struct { size_t mib; int n; } kSpares[] = {{2, 64}, {8, 24}, {32, 8}, {128, 2}};
        for (const auto &sp : kSpares)
            for (int k = 0; k < sp.n; ++k) {
                void *q = nullptr;
                const size_t bytes = sp.mib << 20;
                if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return; }
                (void)hipMemsetAsync(q, 0, bytes, g_ctxStream);
                give(q, bytes);
            }
    }
    std::set<int> warmed;
    // give every cached block of the current device back to the driver (ppg_release_cached_memory; also when hipMalloc fails)
    void trim() {
        int dev = 0; (void)hipGetDevice(&dev);
        std::vector<Block> out;
        {
            std::lock_guard<std::mutex> g(m);
            for (auto &kv : blocks[dev]) { out.push_back(kv.second); held -= kv.first; }
            blocks[dev].clear();
        }
        for (Block &b : out) {
            if (b.ready) { (void)hipEventSynchronize(b.ready); (void)hipEventDestroy(b.ready); }
            (void)hipFree(b.p);
        }
    }
};
static BlockCache g_blockCache;

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    size_t bytes = 0;  // size of the block behind p
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), bytes(o.bytes) { o.p = nullptr; o.cap = 0; o.bytes = 0; }
    ~DevBuf() { if (p) g_blockCache.give(p, bytes); }
    hipError_t reserve(size_t n, bool keep = false) {
        if (n <= cap) return hipSuccess;
        const size_t want = BlockCache::roundUp(std::max(n, cap + cap / 2) * sizeof(T));
        size_t got = 0;
        T *np = (T *)g_blockCache.take(want, got);
        hipError_t e = hipSuccess;
        if (!np) {
            e = hipMalloc(&np, want);
            static const bool debugAlloc = getenv("PPG_DEBUG_ALLOC") != nullptr;  // every block asked of the driver (none in a steady state)
            if (debugAlloc) fprintf(stderr, "[ppg alloc] hipMalloc %zu MiB -> %s (cache holds %zu MiB)\n", want >> 20, e == hipSuccess ? "ok" : "FAILED: cache released", g_blockCache.held >> 20);
            if (e != hipSuccess) {  // memory parked in the cache is memory the driver cannot hand out: release it and try once more
                (void)hipGetLastError();
                g_blockCache.trim();
                e = hipMalloc(&np, want);
                if (e != hipSuccess) return e;
            }
            got = want;
            // touch fresh device memory once, where it is allocated (normally scene set-up), so that whatever the driver does lazily for a new
            // allocation is not paid inside the first render that reaches it: the first process on a freshly booted box sometimes ran a
            // 20-pass render 20-30 % slower than the second.  On the context's own stream when a render is under way.
            (void)hipMemsetAsync(np, 0, want, g_ctxStream);
        }
        if (keep && p && cap) e = hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, g_ctxStream);
        if (keep && p && cap && !g_ctxStream) (void)hipStreamSynchronize(nullptr);
        if (p) g_blockCache.give(p, bytes);
        p = np; bytes = got; cap = got / sizeof(T);
        return e;
    }
};

struct HostSNode {  // host mirror of one S-tree node (STreeNode, GP:740-845)
    int axis = 0;
    uint32_t child[2] = {0, 0};
    bool isLeaf() const { return child[0] == 0; }
};

int parseEnum(const char *s, const char *dflt, std::initializer_list<const char *> names) {
    std::string v = s ? s : dflt;
    int i = 0;
    for (const char *n : names) {
        if (v == n) return i;
        ++i;
    }
    return -1;
}

struct KernelTimer {
    struct Rec { hipEvent_t a, b; int id; uint64_t units; };
    std::vector<std::string> names;
    std::vector<double> ms;
    std::vector<uint64_t> launches, units;
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    bool enabled = false;
    int idOf(const char *n) {
        for (size_t i = 0; i < names.size(); ++i) if (names[i] == n) return (int)i;
        names.push_back(n); ms.push_back(0); launches.push_back(0); units.push_back(0);
        return (int)names.size() - 1;
    }
    hipEvent_t ev() { if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; } hipEvent_t e; (void)hipEventCreate(&e); return e; }
    void resolve() {
        for (auto &r : pending) {
            (void)hipEventSynchronize(r.b);
            float t = 0; (void)hipEventElapsedTime(&t, r.a, r.b);
            ms[r.id] += t; launches[r.id]++; units[r.id] += r.units;
            pool.push_back(r.a); pool.push_back(r.b);
        }
        pending.clear();
    }
    void reset() { resolve(); for (size_t i = 0; i < ms.size(); ++i) { ms[i] = 0; launches[i] = 0; units[i] = 0; } }
};

}  // namespace

// A launch of whole groups of a final iteration's passes (include/ppg.h "Final iteration: groups of passes"): `batch` passes = groups of
// groupPasses passes (the last one may be shorter; or a part of ONE group when groupPasses >= batch), the first starting at pass
// firstPass of the render, consecutive groups of the launch stridePasses apart; group k accumulates into slot slot0 + k * slotStride.
// addCount > 0 (one GPU): the launch's slots are added to image and film right after its film kernel (k_add_groups).
// groupsDone: the launch ends every group it renders (false: a part of one group that later launches continue) — a filtered film resolves
// a group's footprint into its slot then (ppg_set_rfilter) — unless `exchange`: the group is rendered by tiles with a filtered film, and the
// caller resolves it once the ranks have exchanged their footprints' borders (include/ppg.h "Footprint hook").
struct GroupLaunch { unsigned int firstPass, groupPasses, stridePasses, slot0, slotStride; bool wholeFilm; unsigned int addCount; bool groupsDone = true; bool exchange = false; };

struct ppg_ctx {
    // properties (GP:1014-1085)
    int nee = 0, sampleCombination = 1, spatialFilter = 0, directionalFilter = 0, loss = 0, budgetType = 1;
    int sdTreeMaxMemory = -1, sTreeThreshold = 12000, sppPerPass = 4, rrDepth = 5, maxDepth = -1;
    float dTreeThreshold = 0.01f, bsdfSamplingFraction = 0.5f, budget = 300.0f;
    bool dumpSDTree = false, strictNormals = false, hideEmitters = false;
    uint64_t seed = 0;
    int device = 0;
    std::string dumpPrefix, error;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;    // k_commit of the finished paths runs here while k_tail finishes the stragglers on `stream`
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    // The end of a round of the optimiser — k_splat_sorted on stream2, the order / apply kernels on stream3 — runs BESIDE the beginning of the
    // next batch (k_generate and the first k_trace, which need neither the building tree nor the sampling fractions): k_adam_apply is a set
    // of serial chains that leaves most of the GPU idle.  treePending: that work has been enqueued and not yet been waited for; joinTree()
    // makes the context's stream wait for it — before the first kernel that reads the SD-tree or the fractions, and in every entry point.
    hipStream_t stream3 = nullptr;
    hipEvent_t evTreeFork = nullptr, evSplatDone = nullptr, evAdamDone = nullptr;
    bool treePending = false;
    void joinTree() {
        if (!treePending) return;
        (void)hipStreamWaitEvent(stream, evSplatDone, 0);
        (void)hipStreamWaitEvent(stream, evAdamDone, 0);
        treePending = false;
    }
    // Entry points that re-size or release buffers (ppg_set_scene, ppg_set_shard, ppg_begin_render): a render that was cancelled or failed
    // may have left kernels on the side streams that no join has waited for — wait for all of them on the host, then forget what they owed.
    void quiesce() {
        joinTree();
        if (stream2) (void)hipStreamSynchronize(stream2);
        if (stream3) (void)hipStreamSynchronize(stream3);
        if (stream4) (void)hipStreamSynchronize(stream4);
        if (stream) (void)hipStreamSynchronize(stream);
        for (Stragglers &g : strag) { g.pending = false; g.aside = false; g.film = nullptr; }
    }
    // STRAGGLERS (see "Stragglers" below renderBatch's helpers): the handful of paths of a batch that are still alive at depth `defer_depth`
    // leave k_tail, are finished by a second k_tail on stream4 BESIDE the next batch, and what the batch still owes — its film kernel, the
    // stragglers' commit — is done by the next batch (drainStragglers) or at the end of the call (flushStragglers).
    hipStream_t stream4 = nullptr;
    hipEvent_t evStragFork = nullptr, evStragDone = nullptr;
    struct Stragglers {
        DevBuf<float4> rec, vert;           // [cap][8] path records as k_tail wrote them; [maxVertices][n][4 | 6] vertex slots
        DevBuf<unsigned int> orig, iota, ticket, base, origSorted, perm;
        DevBuf<unsigned long long> count;   // [0] stragglers (k_tail's StragOut), as k_tail's `total` afterwards
        DevBuf<unsigned char> nv8;
        DevBuf<float> neeCos, theta;        // theta: the optimiser's variables of the stragglers' round (DevTree::theta_frozen)
        size_t iotaN = 0;
        PathState P{};                      // the compact state: n paths, path j = path orig[j] of the batch
        unsigned int n = 0;
        bool pending = false;               // a batch is owed its film kernel (and its stragglers' commit)
        bool aside = false;                 // ... and their k_tail was put on stream4 (evStragDone)
        bool commit = false, adam = false;  // the stragglers recorded vertices / those leave optimiser records (a round)
        std::function<void()> film;         // the batch's film kernel(s), reading liKeep
    } strag[2];                             // [stragCur]: the set the current batch fills; the other one: the previous batch's, while it is pending
    int stragCur = 0;
    DevBuf<float4> d_liKeep;                // Li of every path of the batch whose film kernel is owed (consumed before the next copy is taken)
    Stragglers &stragPrev() { return strag[stragCur ^ 1]; }
    int tuneSplitDepth = PPG_ADAM_DEFER_DEPTH;  // PPG_SPLIT_DEPTH: the depth at which a batch WITHOUT optimiser records hands its stragglers over (pure
                                                // scheduling: final iterations, renders without a learned fraction; 0 = never).  Rounds of the
                                                // optimiser use PPG_ADAM_DEFER_DEPTH — there the depth is part of the result (include/ppg.h)
    bool tuneFinalHalves = false;               // PPG_FINAL_HALVES: a final iteration that fits one launch is rendered in two (renderFinalGroups)
    // rounds by image region (include/ppg.h ppg_set_adam_regions): the owned pixels grouped by the region of their 32x32 block
    int adamRegions = 0;
    DevBuf<unsigned int> d_regionPixels;
    std::vector<unsigned int> regionOffset;   // [regions + 1] into d_regionPixels
    int regionsBuilt = 0;                     // the lists are valid for this many regions (0: none; reset when the shard or the film changes)
    int deferDepthAdam = PPG_ADAM_DEFER_DEPTH;  // (tests lower it through ppg_debug_set_defer_depth to meet many stragglers in small scenes)
    int joinStragglers() {  // the side stream's work is over as far as the context's stream is concerned (entry points, error paths)
        int rc = 0;
        for (Stragglers &g : strag) if (g.pending && g.aside) { g.aside = false; rc = (int)hipStreamWaitEvent(stream, evStragDone, 0); }
        return rc;
    }
    DevBuf<unsigned char> d_straggler;  // [path] 1 = still alive when the persistent-thread tail took over
    DevBuf<unsigned char> d_nv8;        // [path] vertex slots k_commit takes of the path (k_commit_prepare)

    // scene
    bool haveScene = false;
    bool fullMaterials = false;
    DevBuf<float4> d_tris, d_accel, d_accelSmall, d_normals, d_materials, d_emitters, d_emTris, d_emNrm;
    DevBuf<float> d_rtrans;  // ppg_scene.rtrans (roughplastic slices)
    DevBuf<float4> d_spheres;  // 4 float4 per analytic sphere (DevScene::spheres)
    DevBuf<float2> d_uvs;  // bitmap textures: per-triangle texture coordinates, the texel arrays, the DevTex table
    std::vector<DevBuf<float4>> d_texTexels;
    DevBuf<DevTex> d_textures;
    DevBuf<float4> d_emTexels;  // image-based environment emitter: texels, cdfs, row weights
    DevBuf<float> d_emCdfRows, d_emCdfCols, d_emRowWeights;
    DevBuf<float> d_emSel, d_emArea, d_neeCos;
    DevBuf<int4> d_emInfo;
    DevBuf<BvhNode> d_bvh;
    DevBuf<Bvh4QNode> d_bvh4;
    DevBuf<float4> d_bvhTop;  // BvhBuilder::topCut
    DevScene scene{};
    float aabbMin[3], aabbMax[3];  // Scene::getAABB()
    float geomMin[3], geomMax[3];  // the kd-tree's box (m_kdtree->getAABB()): Scene::getAABB() before the sensor's box is added
    bool lensOn = false;           // ppg_set_lens: thin lens (kept across ppg_set_scene; copied into scene.cam)
    ppg_lens lens{};
    std::vector<ppg_material_textures> materialTextures;  // ppg_set_material_textures: kept until replaced; ppg_set_scene validates and packs it
    std::vector<ppg_delta_emitter> deltaEmitters;  // ppg_set_delta_emitters: kept until replaced; ppg_set_scene builds d_delta from it
    std::vector<ppg_delta_emitter> sceneDelta;     // ... as the scene that is set was built with (ppg_set_lens: the scene box)
    DevBuf<float4> d_delta;
    std::vector<ppg_shape> shapes;  // ppg_set_shapes: kept until replaced; ppg_set_scene validates it and builds d_shapes from it
    DevBuf<float4> d_shapes;
    std::vector<ppg_microfacet> microfacet;  // ppg_set_microfacet: kept until replaced; ppg_set_scene validates it and builds d_mfd from it
    DevBuf<float4> d_mfd;
    std::vector<ppg_coating> coatings;  // ppg_set_coatings: kept until replaced; ppg_set_scene validates it and builds d_coat from it
    DevBuf<float4> d_coat;
    std::vector<ppg_blend> blends;  // ppg_set_blends: kept until replaced; ppg_set_scene validates it and builds d_blend from it
    DevBuf<float4> d_blend;
    // ppg_set_media: kept until replaced (mediaList points into the four vectors; n_media = 0: none); ppg_set_scene validates it and builds
    // d_media and d_primMedia from it.  d_pathMedium: PathState::medium of a scene that binds a medium
    ppg_media mediaList{};
    std::vector<ppg_medium> media;
    std::vector<uint32_t> triMedia, sphereMedia, shapeMedia;
    DevBuf<float4> d_media;
    DevBuf<unsigned int> d_primMedia, d_pathMedium;
    MediaArgs mediaArgs{};         // of the scene that is set: what the media kernels get beside it (all zero: the scene binds no medium)
    // ppg_set_media_volumes: kept until replaced (volumesList points into the vectors; n_entries = 0: none); ppg_set_scene validates it and
    // builds d_volumes, d_volPool and d_het from it
    ppg_media_volumes volumesList{};
    std::vector<ppg_volume> volumes;
    std::vector<std::vector<float>> volumeData;
    std::vector<ppg_medium_volumes> volumeEntries;
    DevBuf<float4> d_volumes, d_het;
    DevBuf<float> d_volPool;
    std::vector<char> hetMedium;   // of the scene that is set: per medium, whether it is heterogeneous
    HetArgs hetArgs{};             // of the scene that is set: what the hetmedia kernels get on top (all zero: no bound medium is heterogeneous)
    uint32_t nMaterials = 0;       // of the scene set last (ppg_debug_bsdf checks its items against it)
    bool renderOpen = false;       // between ppg_begin_render and ppg_end_render
    int W = 0, H = 0;

    // shard
    int shardRank = 0, shardWorld = 1, tileSize = 32;
    bool pathsReady = false;
    int maxBatch = 1;
    DevBuf<unsigned int> d_pixels;
    unsigned int nPix = 0;
    // final iteration of a sharded render: whole groups of passes over ALL pixels instead of all passes over this rank's tiles
    // (include/ppg.h "Final iteration: groups of passes")
    DevBuf<unsigned int> d_pixelsAll;
    unsigned int nPixAll = 0;
    DevBuf<float> d_partials;         // group slots (7 floats per pixel each); sharded: preceded by a film head (4 floats per pixel)
    unsigned int partialSlots = 0;    // slots the buffer holds
    bool partialsPending = false;     // sharded: this rank's slots wait for the exchange (ppg_final_partials / ppg_final_partials_commit)
    bool partialsExported = false;
    unsigned int pendingGroups = 0;
    // reconstruction filter (ppg_set_rfilter): `filtered` = anything but the default box, whose path (own pixel, unit weight: k_film,
    // k_film_groups) stays as it is; a filtered film goes through the footprint partials of k_film_filter / k_film_resolve (ppg_kernels.h)
    bool filtered = false;
    int rfBorder = 0;
    FilmFilter rf{};
    DevBuf<float> d_foot;             // float[(2 rfBorder + 1)^2][7][W * H]: ONE footprint, whatever the batch schedule
    // A filtered film sharded by tiles (include/ppg.h "Footprint hook"): the table of border slots (ppg_kernels.h k_halo_pack), built when
    // the shard, the film or the filter changed (haloKey), the halo buffer the hook all-reduces, and the hook calls of the current
    // ppg_render_passes_nostat call: footDue of them are owed — a number every rank computes alike —, footDone were made.
    ppg_footprint_hook footHook = nullptr;
    void *footHookUser = nullptr;
    DevBuf<unsigned int> d_haloSrc, d_haloPack, d_haloUnpack;
    DevBuf<unsigned char> d_haloTap;
    DevBuf<float> d_halo;             // float[7][haloM]
    unsigned int haloM = 0, haloPackN = 0, haloUnpackN = 0;
    int haloKey[6] = {0, 0, 0, 0, 0, 0};  // width, height, tile size, world, rank, border the table was built for
    unsigned int footDue = 0, footDone = 0;
    bool footFailed = false;          // an exchange carried a failure: every rank saw it there, no further hook calls in this call
    bool exchangesFootprints() const { return filtered && shardWorld > 1; }
    uint64_t samplesLocal = 0;        // samples this rank rendered in the current performRenderPasses

    // path state
    DevBuf<float4> d_ray_o, d_ray_d, d_thr, d_li, d_hit, d_vd, d_vthr, d_vbsdf, d_vrad, d_vo, d_vvox;
    DevBuf<uint4> d_misc;
    DevBuf<float4> d_pathRec, d_vertexRec;  // interleaved layout (PathState Field, ppg_kernels.h): 8 float4 per path, 4 / 6 per vertex slot
    DevBuf<uint4> d_miscCompact;
    bool aosPaths = false;  // the layout in use (allocPaths; PPG_PATH_LAYOUT)
    DevBuf<unsigned int> d_queue[2], d_qcount[2], d_qtotal, d_queueSorted, d_qcommon;
    DevBuf<unsigned char> d_sortKeys;
    int maxBatchFinal = 1;  // passes per batch in the final iteration (nothing is recorded: no vertex slots needed)
    DevBuf<BlockStats> d_stats;
    Queues queues{};
    int nBlocks = 4096;  // persistent workgroups of the path kernels (16 per CU; KITCHEN 720p: 2048 → 76.5, 4096 → 81.3, 8192 → 75.0 Msamples/s)
    PathState paths{};
    int maxVertices = 0;

    // film
    DevBuf<float> d_image, d_sq, d_imageW, d_film, d_filmW, d_var, d_lum, d_tmp;
    float *h_lum = nullptr;  // pinned staging of d_lum (variance sum on the host, finishPasses)
    size_t h_lumCap = 0;
    BlockStats *h_stats = nullptr;  // pinned staging of d_stats
    size_t h_statsCap = 0;
    std::vector<DevBuf<float>> images;  // inverse-variance copies (weight-normalised)
    std::vector<float> variances;

    // SD-tree
    bool treeAlive = false;
    std::vector<HostSNode> snodes;
    std::vector<LeafHdr> hdr;  // host mirror (valid after build / refine)
    std::vector<unsigned int> leaves;
    DevBuf<int4> d_stree;
    DevBuf<LeafHdr> d_hdr;
    DevBuf<SNode> d_snodes[2];
    int cur = 0;  // d_snodes[cur] = sampling pool
    size_t nSamplingNodes = 0, nBuildingNodes = 0;
    DevBuf<ushort4> d_bchild;
    DevBuf<unsigned long long> d_bacc, d_bweight, d_total, d_bweightRep;
    // sampling-fraction optimiser: the records of the current round (include/ppg.h "Learning the BSDF sampling fraction")
    DevBuf<unsigned long long> d_adamKeys[2];
    DevBuf<unsigned int> d_adamIdx[2], d_adamNv, d_adamBase, d_adamCount;
    DevBuf<AdamRec> d_adamRecs, d_adamRecsOut;
    DevBuf<float4> d_splat;       // a round's splat records (k_commit_records), at the positions of the optimiser's records
    bool sortedCommit = false;    // this round commits through records + sort + k_splat_sorted instead of k_commit
    unsigned int adamFlagShift = 0;  // key bit of "a splat only" in such a round: just above the leaf bits
    DevBuf<unsigned char> d_sortTemp, d_orderTemp;
    DevBuf<unsigned int> d_adamLeafCount[2], d_adamLeafOrder[2];  // k_adam_apply's order of the D-trees: most records first
    size_t adamIota = 0;          // d_adamIdx[0][0 .. adamIota) holds the identity permutation
    bool adamFast = false;        // record positions known in advance (DevTree::adam_base)
    bool adamActive = false;      // a round of the optimiser is being rendered
    bool inHook = false, hookReplaced = false;
    uint64_t hookCount = 0;
    int hookPhase = 0;            // 0: before the round's records are applied, 1: after (sharded optimiser, include/ppg.h)
    bool ownerMode = false;       // phase 0 asked for the records by owner: phase 1 follows
    DevBuf<unsigned int> d_adamState;             // [world * segment][6] (ppg_adam_state)
    DevBuf<unsigned long long> d_ownerBounds;     // [world + 1] first record of every owner
    // unbounded paths: live paths after each bulk bounce of the last batch → how many bulk bounces the next batch runs before k_tail
    DevBuf<unsigned int> d_bounceCounts, d_ticket;
    RoundReadback *h_round = nullptr;  // pinned (ppg_batch_plan.h)
    SurvivalCurve survival;           // of the previous batch: sizes the schedule of the next one (planBounces)
    int bounceMargin = 3;             // PPG_BOUNCE_MARGIN: bounces launched beyond the predicted need (the device skips what it does not need)
    // Tuning switches, read ONCE from the environment by ppg_create (DESIGN.md "Tuning switches"); none of them changes a result.
    unsigned int tailThreshold = 0;   // PPG_TAIL_THRESHOLD: live paths below which k_tail takes over (0 = automatic: max(tailMin, paths / tailDiv))
    // PPG_TAIL_MIN, PPG_TAIL_DIV (KITCHEN 720p: 131072 / 16 -> 786432 / 12: +1.5 % at 127 passes, +5 % at 20; with the tail's state in registers
    // a plateau from 1.6 M to 4 M: 786432 -> 2 M another +1.5 % at 20 passes, equal at 127)
    unsigned int tailMin = 2097152, tailDiv = 12;
    size_t tuneBatchPaths = 0;        // PPG_BATCH_PATHS: paths in flight per batch of passes (0 = automatic)
    int tuneBlocks = 0;               // PPG_BLOCKS: persistent workgroups of the path kernels (0 = 4096)
    bool tuneForceBvh = false;        // PPG_FORCE_BVH: trace small scenes through the BVH as well
    bool tuneNoSort = false;          // PPG_NO_SORT: do not sort the queue slices by BSDF type before k_shade<FULL>
    bool tuneNoSortFirst = false;     // PPG_NO_SORT_FIRST: the first bounce of a batch unsorted through the complete k_shade<FULL>
    bool tuneNoSplit = false;         // PPG_NO_SPLIT: one k_shade<FULL> over the whole sorted slice instead of k_shade<.., MSET_COMMON> + the rest
    bool tuneNoOverlap = false;       // PPG_NO_OVERLAP: k_commit after k_tail on one stream instead of beside it
    bool tuneNoSortedCommit = false;  // PPG_NO_SORTED_COMMIT: a round of the optimiser commits with k_commit (global atomics) instead of records + sort + k_splat_sorted
    unsigned int tuneSplatLdsNodes = PPG_SPLAT_NODES;  // PPG_SPLAT_LDS_NODES: k_splat_sorted stages D-trees of up to this many nodes in LDS (<= PPG_SPLAT_NODES)
    bool tuneNoAside = false;         // PPG_NO_ASIDE: the optimiser's order / apply kernels stay on the context's stream (k_splat_sorted still runs beside them)
    bool tuneAdamUnordered = false;   // PPG_ADAM_UNORDERED: k_adam_apply takes the D-trees in leaf order instead of busiest first
    int tuneBulkBounces = -1;         // PPG_BULK_BOUNCES: fixed number of wavefront bounces before k_tail takes over (-1 = adaptive)
    bool debugBatch = false;          // PPG_DEBUG_BATCH: one line per batch on stderr (paths, live paths after every bulk bounce, tail time)
    int tuneFinalBatch = 0;           // PPG_FINAL_BATCH: passes per batch of the final iteration (0 = 64)
    int tuneTailBlocks = 0;           // PPG_TAIL_BLOCKS: workgroups of k_tail when k_commit runs beside it (0 = automatic)
    int tunePathLayout = 0;           // PPG_PATH_LAYOUT = soa (1) | aos (2): layout of the per-path state (0 = automatic, allocPaths)
    int tuneBlocksSmall = 2048;       // PPG_BLOCKS_SMALL: workgroups of the wavefront kernels for batches of at most tuneSmallPaths paths (0 = nBlocks for every batch)
    size_t tuneSmallPaths = 13000000; // PPG_SMALL_PATHS.  KITCHEN 720p (r06_experiments.json s23, s27): 2048 for batches up to 4 M / 16 M / 32 M paths: +0.1 / +1.1 / +1.2 % on the
                                      // driver's command (its final iteration is one batch of 12 M), +0.2 % at 127 passes, -0.3 % at 1023 with 16 M (its 14.7 M-path rounds): 13 M
    int tuneBvhLeaf = 4;              // PPG_BVH_LEAF: triangles per BVH leaf (1..8).  KITCHEN 720p, driver's command: 4 -> 3 +3.5 % once the node test had become
                                      // cheap (130.9 -> 135.6, A/B on one box; with the world-space decode 2 / 3 / 4 / 6 / 8 gave 125.8 / 125.9 / 124.5 / 119.6 / 115.2)
    float tuneBvhPad = 2e-6f;         // PPG_BVH_PAD: box padding relative to the scene extent
    bool tuneNoTopCut = false;        // PPG_NO_TOPCUT: trace_closest4_wave starts at the root instead of the top cut
    DevBuf<unsigned int> d_leaves, d_counts, d_offsets, d_grid;
    DevBuf<unsigned int> d_dfs[2], d_refEv, d_refLv, d_refEvOff, d_refLvOff;  // S-tree refine: leaves in the reference's (right-first) visiting order
    int dfsCur = 0;
    unsigned int dfsCount = 0;
    int ldsNodes = 0, ldsTris = 0;  // scene part cached in LDS by k_trace
    float treeMin[3], treeMax[3], treeExt[3];
    bool isBuilt = false, isFinalIter = false, doNee = false;
    bool iterOpen = false;  // between ppg_begin_iteration(ctx, 0) and ppg_build_sdtree: the building tree takes records (ppg_debug_commit)
    int iter = 0, passesRendered = 0, passesRenderedThisIter = 0, passesLocal = 0;
    std::chrono::steady_clock::time_point startTime, passStart;
    std::atomic<bool> cancelled{false};
    bool cancelSeen = false;  // the render under way has acted on the flag (seesCancel): ppg_begin_render then does not apply it to the next one
    bool seesCancel() { if (!cancelled.load()) return false; cancelSeen = true; return true; }
    float lastVariance = 0;
    ppg_pass_stats lastStats{};
    KernelTimer timer;
#define PPG_TAIL_LOG 256
    DevBuf<unsigned int> d_tailLongest;  // [PPG_TAIL_LOG] longest path (bounces) finished by each k_tail launch of the current performRenderPasses
    unsigned int tailLaunches = 0;
    uint64_t tailLongestSum = 0;  // sum over all k_tail launches of the longest path each finished (bounces): the tails' critical path
    uint64_t shadeCommonRays = 0;  // rays through k_shade<.., MSET_COMMON> while kernel timing is on
    uint64_t bvhNodesVisited = 0, bvhTrisTested = 0;  // by k_trace while kernel timing is on (the roofline's node / triangle counts)
    ppg_pass_hook passHook = nullptr;
    void *passHookUser = nullptr;
    ppg_stop_hook stopHook = nullptr;
    void *stopHookUser = nullptr;
#ifdef PPG_PROBE
    DevBuf<unsigned long long> d_probe;  // development builds: cycle sums of the lone path's bounce (ppg_kernels.h PROBE_MARK), printed by endRender
#endif

    DevTree devTree() {
        DevTree T{};
        T.stree = d_stree.p; T.hdr = d_hdr.p; T.snodes = d_snodes[cur].p; T.bchild = d_bchild.p; T.bacc = d_bacc.p;
        T.bweight = d_bweight.p;
        T.bweight_rep = d_bweightRep.p;
        T.adam_keys = adamActive ? d_adamKeys[0].p : nullptr; T.adam_recs = adamActive ? d_adamRecs.p : nullptr;
        T.adam_count = d_adamCount.p; T.adam_base = (adamActive && adamFast) ? d_adamBase.p : nullptr;
        T.adam_cap = adamActive ? (unsigned int)std::min<size_t>(std::min(d_adamRecs.cap, d_adamKeys[0].cap), 0xfffffff0u) : 0u;  // (both are written at the same position)
        for (int a = 0; a < 3; ++a) { T.aabb_min[a] = treeMin[a]; T.aabb_ext[a] = treeExt[a]; T.aabb_max[a] = treeMax[a]; }
        T.is_built = isBuilt ? 1 : 0;
        T.grid = d_grid.p;
        return T;
    }
    RenderParams params() const {
        RenderParams R{};
        R.nee = nee; R.spatial_filter = spatialFilter; R.directional_filter = directionalFilter; R.loss = loss;
        R.bsdf_sampling_fraction = bsdfSamplingFraction; R.rr_depth = rrDepth; R.max_depth = maxDepth;
        R.strict_normals = strictNormals; R.hide_emitters = hideEmitters; R.spp = sppPerPass;
        R.is_final_iter = isFinalIter; R.do_nee = doNee; R.seed = seed; R.pass_index = (unsigned int)passesRendered;
        R.max_vertices = maxVertices; R.img_pixels = (unsigned int)W * (unsigned int)H;
#ifdef PPG_PROBE
        R.probe = d_probe.p;
#endif
        return R;
    }
};

PathKernels ppg_path_kernels[PPG_FAMILIES];  // filled by the units of ppg_inst.hip when the library is loaded

// The kernel family a scene runs: the lowest that has everything the scene needs (ppg_device.h).
static int sceneFamily(const DevScene &S, const MediaArgs &M, const HetArgs &V) {
    if (V.het) return PPG_FAMILY_HETMEDIA;     // a bound medium is heterogeneous: the top family, whatever else the scene holds
    if (M.media) return PPG_FAMILY_MEDIA;      // a medium is bound to a primitive or to the camera: the media family, whatever else the scene holds
    if (S.lobes) return PPG_FAMILY_LOBES;      // a roughdiffuse, difftrans or phong material, a normal-mapped or a null one: the top family, whatever else the scene holds
    if (S.blend) return PPG_FAMILY_BLEND;      // a blended material: the blend family, whatever else the scene holds
    if (S.coat) return PPG_FAMILY_COAT;        // a coated material: the coat family, shapes and general entries or not
    if (S.mfd) return PPG_FAMILY_EXT;          // a general microfacet entry: the extended family, shapes or not
    if (S.n_shapes) return PPG_FAMILY_SHAPES;  // an analytic disk or cylinder
    return PPG_FAMILY_BASE;                    // (only here is a scene ever small, or without the FULL material set)
}
// a launcher of the table; one that no unit has entered is a fault in the build of the library
template <typename F> static F launcher(F f) {
    if (!f) { fprintf(stderr, "libppg_hip: no unit of this library holds the kernel asked for\n"); abort(); }
    return f;
}
// variant = (NEE ? 2 : 0) | (FULL ? 1 : 0)
static void ppg_launch_shade(int variant, const ShadeLaunch &a) { launcher(ppg_path_kernels[sceneFamily(a.S, a.M, a.V)].shade[variant >> 1])(variant, a); }
// variant = (SMALL ? 4 : 0) | (NEE ? 2 : 0) | (FULL ? 1 : 0)
static void ppg_launch_tail(int variant, const TailLaunch &a) { launcher(ppg_path_kernels[sceneFamily(a.S, a.M, a.V)].tail[variant >> 1])(variant, a); }
// the scene is traced from LDS without a BVH (k_trace<true>, k_tail<true, ..>)
static bool isSmallScene(const ppg_ctx *ctx) {
    return ctx->scene.n_tris <= 64 && ctx->ldsTris == ctx->scene.n_tris && ctx->scene.n_spheres == 0 && sceneFamily(ctx->scene, ctx->mediaArgs, ctx->hetArgs) == PPG_FAMILY_BASE && !ctx->tuneForceBvh;
}
namespace {

template <typename F> void timedLaunch(ppg_ctx *ctx, const char *name, uint64_t units, F &&launch) {
    if (!ctx->timer.enabled) { launch(); return; }
    KernelTimer::Rec r; r.a = ctx->timer.ev(); r.b = ctx->timer.ev(); r.id = ctx->timer.idOf(name); r.units = units;
    (void)hipEventRecord(r.a, ctx->stream);
    launch();
    (void)hipEventRecord(r.b, ctx->stream);
    ctx->timer.pending.push_back(r);
}

bool sideStreamsAllowed(const ppg_ctx *ctx) { return ppg_plan::sideStreamsAllowed(ctx->timer.enabled, ctx->tuneNoOverlap); }

int gridFor(size_t n, int block = PPG_BLOCK, int maxBlocks = 256 * 8) {
    size_t b = (n + block - 1) / block;
    return (int)std::max<size_t>(1, std::min<size_t>(b, (size_t)maxBlocks));
}

float elapsedSeconds(std::chrono::steady_clock::time_point start) {  // GP:1428-1432
    auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - start);
    return (float)ms.count() / 1000;
}

// nodes: also copy the S-tree nodes and leaf headers host → device (only needed when the host mirror is the newer copy, i.e. for the
// single root node at the start of a render; afterwards the device refines the tree and the host mirror is downloaded from it)
int uploadTree(ppg_ctx *ctx, bool nodes) {
    size_t n = ctx->snodes.size();
    std::vector<int4> st(nodes ? n : 0);
    if (nodes) {
        for (size_t i = 0; i < n; ++i) st[i] = make_int4(ctx->snodes[i].axis, (int)ctx->snodes[i].child[0], (int)ctx->snodes[i].child[1], 0);
        HIP_CHECK(ctx->d_stree.reserve(n));
        HIP_CHECK(ctx->d_hdr.reserve(n));
        HIP_CHECK(hipMemcpyAsync(ctx->d_stree.p, st.data(), n * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(ctx->d_hdr.p, ctx->hdr.data(), n * sizeof(LeafHdr), hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->leaves.clear();
    for (size_t i = 0; i < n; ++i) if (ctx->snodes[i].isLeaf()) ctx->leaves.push_back((unsigned int)i);
    HIP_CHECK(ctx->d_leaves.reserve(ctx->leaves.size()));
    HIP_CHECK(ctx->d_counts.reserve(ctx->leaves.size()));
    HIP_CHECK(ctx->d_offsets.reserve(ctx->leaves.size()));
    HIP_CHECK(hipMemcpyAsync(ctx->d_leaves.p, ctx->leaves.data(), ctx->leaves.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(ctx->d_bweight.reserve(n));
    HIP_CHECK(hipMemsetAsync(ctx->d_bweight.p, 0, n * 8, ctx->stream));
    HIP_CHECK(ctx->d_bweightRep.reserve(n * PPG_REPLICAS));
    HIP_CHECK(hipMemsetAsync(ctx->d_bweightRep.p, 0, n * PPG_REPLICAS * 8, ctx->stream));
    if (n >= (1u << 27)) { ctx->error = "S-tree exceeds 2^27 nodes"; return PPG_ERR_NOMEM; }
    const unsigned int cells = PPG_GRID_DIM * PPG_GRID_DIM * PPG_GRID_DIM;
    HIP_CHECK(ctx->d_grid.reserve(cells));
    hipLaunchKernelGGL(k_build_grid, dim3((cells + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_stree.p, ctx->d_grid.p);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // st is a stack-local staging buffer
    return PPG_OK;
}

// The depth of an S-tree and whether the box spatial filter's splat can walk it: ppg_sdt_load.h (the import of a dumped tree asks the same).
using ppg_sdt::streeDepthCheck;

// STree::refine (GP:957-998) + subdivide (GP:876-895) on the device (k_refine_count → scans → k_refine_fill, ppg_kernels.h);
// the host mirror (node array, leaf headers) is then downloaded — it feeds the statistics log, the dumps and the readers.
int refineDevice(ppg_ctx *ctx, size_t sTreeThreshold, int maxMB) {
    auto &nodes = ctx->snodes;
    auto &hdr = ctx->hdr;
    if (maxMB >= 0) {
        size_t foot = 0;  // approxMemoryFootprint with the reference's sizeof (QuadTreeNode 24 B, DTree 40 B)
        for (size_t i = 0; i < nodes.size(); ++i) foot += nodes[i].isLeaf() ? ((size_t)hdr[i].b_num * 24 + 40) + ((size_t)hdr[i].s_num * 24 + 40) : 2 * (24 + 40);
        if (foot / 1000000 >= (size_t)maxMB) return PPG_OK;
    }
    const unsigned int nl = ctx->dfsCount, nOld = (unsigned int)nodes.size();
    hipStream_t s = ctx->stream;
    HIP_CHECK(ctx->d_refEv.reserve(nl)); HIP_CHECK(ctx->d_refLv.reserve(nl)); HIP_CHECK(ctx->d_refEvOff.reserve(nl)); HIP_CHECK(ctx->d_refLvOff.reserve(nl));
    HIP_CHECK(ctx->d_total.reserve(2));
    hipLaunchKernelGGL(k_refine_count, dim3((nl + 255) / 256), dim3(256), 0, s, ctx->d_hdr.p, ctx->d_dfs[ctx->dfsCur].p, nl, (float)sTreeThreshold,
                       ctx->d_refEv.p, ctx->d_refLv.p);
    hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, s, ctx->d_refEv.p, ctx->d_refEvOff.p, nl, ctx->d_total.p);
    hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, s, ctx->d_refLv.p, ctx->d_refLvOff.p, nl, ctx->d_total.p + 1);
    unsigned long long totals[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(totals, ctx->d_total.p, 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (totals[0] == 0) return PPG_OK;  // no leaf exceeded the threshold
    const unsigned long long nNew = (unsigned long long)nOld + 2ull * totals[0];
    if (nNew >= (1ull << 27)) { ctx->error = "S-tree exceeds 2^27 nodes"; return PPG_ERR_NOMEM; }
    HIP_CHECK(ctx->d_stree.reserve((size_t)nNew, true));
    HIP_CHECK(ctx->d_hdr.reserve((size_t)nNew, true));
    HIP_CHECK(ctx->d_dfs[ctx->dfsCur ^ 1].reserve((size_t)totals[1]));
    hipLaunchKernelGGL(k_refine_fill, dim3(nl), dim3(256), 0, s, ctx->d_stree.p, ctx->d_hdr.p, ctx->d_dfs[ctx->dfsCur].p, nl, nOld, ctx->d_refEv.p,
                       ctx->d_refEvOff.p, ctx->d_refLvOff.p, ctx->d_dfs[ctx->dfsCur ^ 1].p);
    ctx->dfsCur ^= 1;
    ctx->dfsCount = (unsigned int)totals[1];
    std::vector<int4> st((size_t)nNew);
    hdr.resize((size_t)nNew);
    HIP_CHECK(hipMemcpyAsync(st.data(), ctx->d_stree.p, st.size() * sizeof(int4), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(hdr.data(), ctx->d_hdr.p, hdr.size() * sizeof(LeafHdr), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    nodes.resize((size_t)nNew);
    for (size_t i = 0; i < nodes.size(); ++i) { nodes[i].axis = st[i].x; nodes[i].child[0] = (uint32_t)st[i].y; nodes[i].child[1] = (uint32_t)st[i].z; }
    if (ctx->spatialFilter == SF_BOX) {  // stree_record_box walks this tree with a stack of 96 entries (DESIGN.md "Stack bounds of the splats")
        std::vector<uint32_t> ch(2 * nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i) { ch[2 * i] = nodes[i].child[0]; ch[2 * i + 1] = nodes[i].child[1]; }
        uint32_t depth = 0;
        const int rc = streeDepthCheck(ch.data(), (uint32_t)nodes.size(), ctx->spatialFilter, &depth);
        if (rc == PPG_ERR_INVALID) { ctx->error = "internal: an S-tree child that is not above its parent"; return PPG_ERR_STATE; }
        if (rc) { ctx->error = "S-tree deeper than " + std::to_string(PPG_STREE_MAX_DEPTH) + " levels (" + std::to_string(depth) + ") with the box spatial filter"; return rc; }
    }
    return PPG_OK;
}

int resetSDTree(ppg_ctx *ctx) {  // GP:1108-1113
    ctx->joinTree();
    double thr = std::sqrt(std::ldexp(1.0, ctx->iter) * ctx->sppPerPass / 4) * ctx->sTreeThreshold;
    int rc = refineDevice(ctx, (size_t)thr, ctx->sdTreeMaxMemory);
    if (rc) return rc;
    rc = uploadTree(ctx, false);
    if (rc) return rc;
    unsigned int nl = (unsigned int)ctx->leaves.size();
    HIP_CHECK(ctx->d_total.reserve(1));
    DevTree T = ctx->devTree();
    int blocks = (int)((nl + 127) / 128);
    timedLaunch(ctx, "k_dtree_reset<count>", nl, [&] {
        hipLaunchKernelGGL(k_dtree_reset<false>, dim3(blocks), dim3(128), 0, ctx->stream, T, ctx->d_leaves.p, nl, 20, ctx->dTreeThreshold,
                           ctx->d_counts.p, (ushort4 *)nullptr);
    });
    hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, ctx->stream, ctx->d_counts.p, ctx->d_offsets.p, nl, ctx->d_total.p);
    unsigned long long total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, ctx->d_total.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (total > 0xfffffff0ull) { ctx->error = "building D-tree pool exceeds 2^32 nodes"; return PPG_ERR_NOMEM; }
    ctx->nBuildingNodes = (size_t)total;
    HIP_CHECK(ctx->d_bchild.reserve(total));
    HIP_CHECK(ctx->d_bacc.reserve(total * 4));
    HIP_CHECK(ctx->d_snodes[ctx->cur ^ 1].reserve(total));
    HIP_CHECK(hipMemsetAsync(ctx->d_bacc.p, 0, total * 4 * 8, ctx->stream));
    hipLaunchKernelGGL(k_assign_blocks, dim3(blocks), dim3(128), 0, ctx->stream, T, ctx->d_leaves.p, nl, ctx->d_counts.p, ctx->d_offsets.p);
    T = ctx->devTree();
    timedLaunch(ctx, "k_dtree_reset<fill>", nl, [&] {
        hipLaunchKernelGGL(k_dtree_reset<true>, dim3(blocks), dim3(128), 0, ctx->stream, T, ctx->d_leaves.p, nl, 20, ctx->dTreeThreshold,
                           ctx->d_counts.p, ctx->d_bchild.p);
    });
    HIP_CHECK(hipGetLastError());
    return PPG_OK;
}

int foldWeights(ppg_ctx *ctx) {
    ctx->joinTree();
    unsigned int nn = (unsigned int)ctx->snodes.size();
    if (!ctx->d_bweightRep.p || nn == 0) return PPG_OK;
    hipLaunchKernelGGL(k_fold_replicas, dim3((nn + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_bweight.p, ctx->d_bweightRep.p, nn);
    HIP_CHECK(hipGetLastError());
    return PPG_OK;
}

int buildSDTree(ppg_ctx *ctx, ppg_tree_stats *st) {  // GP:1115-1189
    ctx->joinTree();  // (the last round's splats and optimiser steps may still be running beside the context's stream)
    { int rc = foldWeights(ctx); if (rc) return rc; }
    unsigned int nl = (unsigned int)ctx->leaves.size();
    DevTree T = ctx->devTree();
    int blocks = (int)((nl + 127) / 128);
    timedLaunch(ctx, "k_dtree_build", nl, [&] {
        hipLaunchKernelGGL(k_dtree_build, dim3(blocks), dim3(128), 0, ctx->stream, T, ctx->d_leaves.p, nl, ctx->d_snodes[ctx->cur ^ 1].p);
    });
    HIP_CHECK(hipGetLastError());
    ctx->cur ^= 1;  // sampling = building
    ctx->nSamplingNodes = ctx->nBuildingNodes;
    HIP_CHECK(hipMemcpyAsync(ctx->hdr.data(), ctx->d_hdr.p, ctx->hdr.size() * sizeof(LeafHdr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // statistics, in S-tree node order like forEachDTreeWrapperConst (GP:1138-1174)
    int maxDepth = 0, minDepth = std::numeric_limits<int>::max();
    float avgDepth = 0, maxAvgRadiance = 0, minAvgRadiance = std::numeric_limits<float>::max(), avgAvgRadiance = 0;
    size_t maxNodes = 0, minNodes = std::numeric_limits<size_t>::max();
    float avgNodes = 0, maxSW = 0, minSW = std::numeric_limits<float>::max(), avgSW = 0;
    int nPoints = 0, nPointsNodes = 0;
    uint64_t totalNodes = 0;
    for (unsigned int leaf : ctx->leaves) {
        const LeafHdr &h = ctx->hdr[leaf];
        const int depth = h.s_depth;
        maxDepth = std::max(maxDepth, depth); minDepth = std::min(minDepth, depth); avgDepth += depth;
        float avgRadiance = 0;
        if (h.s_statw != 0) { const float factor = 1 / (PPG_PI_F * 4 * h.s_statw); avgRadiance = factor * h.s_sum; }
        maxAvgRadiance = ppg_max(maxAvgRadiance, avgRadiance); minAvgRadiance = ppg_min(minAvgRadiance, avgRadiance);
        avgAvgRadiance += avgRadiance;
        if (h.s_num > 1) {
            const size_t nodes = h.s_num;
            maxNodes = std::max(maxNodes, nodes); minNodes = std::min(minNodes, nodes); avgNodes += nodes; ++nPointsNodes;
        }
        totalNodes += h.s_num;
        maxSW = ppg_max(maxSW, h.s_statw); minSW = ppg_min(minSW, h.s_statw); avgSW += h.s_statw;
        ++nPoints;
    }
    if (nPoints > 0) {
        avgDepth /= nPoints; avgAvgRadiance /= nPoints;
        if (nPointsNodes > 0) avgNodes /= nPointsNodes;
        avgSW /= nPoints;
    }
    if (st) {
        st->min_depth = minDepth; st->max_depth = maxDepth; st->avg_depth = avgDepth;
        st->min_mean_radiance = minAvgRadiance; st->avg_mean_radiance = avgAvgRadiance; st->max_mean_radiance = maxAvgRadiance;
        st->min_nodes = minNodes; st->max_nodes = maxNodes; st->avg_nodes = avgNodes;
        st->min_stat_weight = minSW; st->avg_stat_weight = avgSW; st->max_stat_weight = maxSW;
        st->n_leaves = (uint32_t)nPoints; st->n_stree_nodes = (uint32_t)ctx->snodes.size(); st->n_dtree_nodes = totalNodes;
    }
    ctx->isBuilt = true;
    ctx->iterOpen = false;
    return PPG_OK;
}

int allocPaths(ppg_ctx *ctx) {
    // owned pixel list
    std::vector<unsigned int> pix;
    int tilesX = (ctx->W + ctx->tileSize - 1) / ctx->tileSize;
    for (int y = 0; y < ctx->H; ++y)
        for (int x = 0; x < ctx->W; ++x) {
            int t = (y / ctx->tileSize) * tilesX + (x / ctx->tileSize);
            if (ctx->shardWorld <= 1 || t % ctx->shardWorld == ctx->shardRank) pix.push_back((unsigned int)(y * ctx->W + x));
        }
    ctx->nPix = (unsigned int)pix.size();
    ctx->regionsBuilt = 0;
    HIP_CHECK(ctx->d_pixels.reserve(std::max<size_t>(1, pix.size())));
    if (!pix.empty()) HIP_CHECK(hipMemcpy(ctx->d_pixels.p, pix.data(), pix.size() * 4, hipMemcpyHostToDevice));
    ctx->nPixAll = (unsigned int)((size_t)ctx->W * ctx->H);
    if (ctx->shardWorld > 1) {  // the final iteration's groups are rendered over the whole film
        std::vector<unsigned int> all(ctx->nPixAll);
        for (unsigned int k = 0; k < ctx->nPixAll; ++k) all[k] = k;
        HIP_CHECK(ctx->d_pixelsAll.reserve(std::max<size_t>(1, all.size())));
        if (!all.empty()) HIP_CHECK(hipMemcpy(ctx->d_pixelsAll.p, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    }
    // Pass batching: the passes of an iteration are independent (frozen sampling tree, accumulate-only building
    // tree), so up to maxBatch of them run as ONE set of launches over nPix * spp * batch paths.  Sample indices,
    // per-pixel accumulation order and all integer statistics are unchanged, i.e. results are bit-identical; what
    // changes is that small images / tile shards (multi-GPU strong scaling) still fill the GPU and that the serial
    // tail of unbounded paths is paid once per batch.  When the BSDF sampling fraction is learned, a batch is one
    // ROUND of the optimiser (include/ppg.h: ppg_adam_round_passes — part of the algorithm, not a tuning knob).
    // With a time budget and no rounds the clock is checked after every pass, as in the reference (GP:1259-1262).
    {
        const size_t perPass = std::max<size_t>(1, (size_t)ctx->nPix * ctx->sppPerPass);
        size_t target = 16u << 20;  // ~16 M paths in flight (measured on cbox-720p: 4 M 996, 8 M 1007, 16 M 1034, 32 M 1041 Msamples/s)
        {   // ... but at most ~24 GB of vertex slots (288 GB HBM: ample, this only bounds allocation time)
            int slots = PPG_MAX_VERTICES;
            if (ctx->maxDepth > 0) slots = std::max(1, std::min(PPG_MAX_VERTICES, ctx->maxDepth - 1));
            const size_t perPath = (size_t)slots * (ctx->spatialFilter != SF_NEAREST ? 96 : 64) + 96;
            target = std::min<size_t>(target, (size_t)24e9 / perPath);
        }
        if (ctx->tuneBatchPaths) target = ctx->tuneBatchPaths;
        ctx->maxBatch = ctx->budgetType == 1 ? 1 : (int)std::max<size_t>(1, std::min<size_t>(64, target / perPass));
        if (ctx->loss != LOSS_NONE) {
            // bit PPG_ADAM_PATH_BITS - 1 of the key's path field is PPG_ADAM_DEFER_PATH_BIT (include/ppg.h "Limits")
            if ((uint64_t)ctx->W * ctx->H * ctx->sppPerPass > (uint64_t)PPG_ADAM_DEFER_PATH_BIT) { ctx->error = "width * height * sppPerPass exceeds 2^26 = 67108864 with a bsdfSamplingFractionLoss"; return PPG_ERR_INVALID; }
            ctx->maxBatch = std::max(ctx->maxBatch, (int)ppg_adam_round_passes(ctx->sppPerPass, ctx->W, ctx->H, 1 << 30));
        }
    }
    {   // the final iteration records nothing: its batches need path state only (96 B per path), so they can be larger — the serial tail of
        // unbounded paths is then paid once per 64 passes
        const size_t perPass = std::max<size_t>(1, (size_t)(ctx->shardWorld > 1 ? ctx->nPixAll : ctx->nPix) * ctx->sppPerPass);
        // PPG_FINAL_BATCH=256 (2^28 paths): KITCHEN 700x400 at 2400 spp 5.2 -> 4.9 s, 720p at 511 passes 169 -> 175 Msamples/s — but the 23 GB of
        // path state it sizes cost the FIRST process on a freshly booted GPU box 20 % of a 20-pass render (86 vs 110 Msamples/s; the second
        // process is at par), so the default stays at 64 passes.
        const size_t capPasses = ctx->tuneFinalBatch ? (size_t)ctx->tuneFinalBatch : 64, capPaths = (size_t)1 << (capPasses > 64 ? 28 : 26);
        ctx->maxBatchFinal = ctx->budgetType == 1 ? 1 : (int)std::max<size_t>((size_t)ctx->maxBatch, std::min<size_t>(capPasses, capPaths / perPass));
        if (ctx->tuneBatchPaths) ctx->maxBatchFinal = ctx->maxBatch;
    }
    size_t n = (size_t)ctx->nPix * ctx->sppPerPass * (size_t)ctx->maxBatch;
    const size_t nFinal = (size_t)(ctx->shardWorld > 1 ? ctx->nPixAll : ctx->nPix) * ctx->sppPerPass * (size_t)ctx->maxBatchFinal;
    if (n > 0xfffffff0ull || nFinal > 0xfffffff0ull) { ctx->error = "too many paths per pass"; return PPG_ERR_INVALID; }
    const size_t nTrain = std::max<size_t>(1, n);  // vertex slots: training batches only
    size_t nn = std::max<size_t>(1, std::max(n, nFinal));
    ctx->maxVertices = PPG_MAX_VERTICES;
    if (ctx->maxDepth > 0) ctx->maxVertices = std::max(1, std::min(PPG_MAX_VERTICES, ctx->maxDepth - 1));
    // layout of the per-path state: one array per field (soa) or interleaved 128-byte records (aos).  Interleaving
    // helps the late, scattered bounces — after compaction and the sort by material a lane holds an arbitrary path, and five 16-byte accesses
    // to five arrays cost five sectors — and hurts the early, coalesced ones.  Measured on MI355X, round 4 (profiles/r04_experiments.json,
    // Msamples/s soa / aos): KITCHEN 1023 passes 202 / 209, 127 passes 183 / 187, 20 passes equal; torus-class 1080p 129 / 142; SPACESHIP 1080p
    // 1008 / 874; cbox-720p 1350 / 1038.  So: interleaved for paths of unbounded depth over a BVH scene (long random walks: most bounces are
    // late ones), one array per field otherwise; PPG_PATH_LAYOUT = soa | aos overrides.
    ctx->aosPaths = ctx->tunePathLayout ? ctx->tunePathLayout == 2 : (ctx->maxDepth < 0 && ctx->scene.n_tris > 64);
    if (ctx->aosPaths) { HIP_CHECK(ctx->d_pathRec.reserve(nn * 8)); HIP_CHECK(ctx->d_miscCompact.reserve(nn)); }
    else {
        HIP_CHECK(ctx->d_ray_o.reserve(nn)); HIP_CHECK(ctx->d_ray_d.reserve(nn)); HIP_CHECK(ctx->d_thr.reserve(nn));
        HIP_CHECK(ctx->d_li.reserve(nn)); HIP_CHECK(ctx->d_hit.reserve(nn)); HIP_CHECK(ctx->d_misc.reserve(nn));
    }
    if (ctx->tuneBlocks) ctx->nBlocks = ctx->tuneBlocks;
    const size_t nb = (size_t)ctx->nBlocks;
    const size_t chunks = (nn + PPG_DCHUNK - 1) / PPG_DCHUNK;  // (PPG_DCHUNK is a multiple of PPG_CHUNK: covers the first bounce's dealing too)
    const size_t cap = ((chunks + nb - 1) / nb) * PPG_DCHUNK;
    for (int k = 0; k < 2; ++k) { HIP_CHECK(ctx->d_queue[k].reserve(cap * nb)); HIP_CHECK(ctx->d_qcount[k].reserve(nb)); }
    HIP_CHECK(ctx->d_stats.reserve(nb)); HIP_CHECK(ctx->d_qtotal.reserve(1));
    // k_scan_counts / k_gather_slices write one offset per persistent workgroup and the live count: these two buffers are otherwise sized by
    // the SD-tree code (one entry per S-tree leaf — a single one in the first iteration)
    HIP_CHECK(ctx->d_offsets.reserve(nb)); HIP_CHECK(ctx->d_total.reserve(2));
    HIP_CHECK(ctx->d_bounceCounts.reserve(72)); HIP_CHECK(ctx->d_ticket.reserve(1));
    HIP_CHECK(ctx->d_adamCount.reserve(2));
    if (!ctx->h_round) HIP_CHECK(hipHostMalloc((void **)&ctx->h_round, sizeof(RoundReadback), hipHostMallocDefault));
    ctx->queues.items[0] = ctx->d_queue[0].p; ctx->queues.items[1] = ctx->d_queue[1].p;
    ctx->queues.count[0] = ctx->d_qcount[0].p; ctx->queues.count[1] = ctx->d_qcount[1].p;
    ctx->queues.cap = (unsigned int)cap; ctx->queues.stats = ctx->d_stats.p; ctx->queues.n_blocks = (unsigned int)nb;
    ctx->queues.n_common = nullptr;
    if (ctx->fullMaterials && !ctx->tuneNoSort) {
        HIP_CHECK(ctx->d_queueSorted.reserve(cap * nb)); HIP_CHECK(ctx->d_sortKeys.reserve(cap * nb));
        // (not with media: the kernel of the common classes lies outside the families and knows no medium branch)
        if (!ctx->tuneNoSplit && !ctx->mediaArgs.media) { HIP_CHECK(ctx->d_qcommon.reserve(nb)); ctx->queues.n_common = ctx->d_qcommon.p; }
    }
    size_t nv = nTrain * (size_t)ctx->maxVertices;
    const bool filtered = ctx->spatialFilter != SF_NEAREST;
    PathState &P = ctx->paths;
    P.n_paths = (unsigned int)n; P.n_pix = ctx->nPix; P.pixels = ctx->d_pixels.p;
    if (ctx->aosPaths) {
        const unsigned int vs = filtered ? 6u : 4u;
        HIP_CHECK(ctx->d_vertexRec.reserve(nv * vs));
        float4 *r = ctx->d_pathRec.p, *v = ctx->d_vertexRec.p;
        P.ray_o = {r, 8}; P.ray_d = {r + 1, 8}; P.thr = {r + 2, 8}; P.li = {r + 3, 8}; P.hit = {r + 4, 8}; P.misc = {reinterpret_cast<uint4 *>(r + 5), 8};
        P.v_d = {v, vs}; P.v_thr = {v + 1, vs}; P.v_bsdf = {v + 2, vs}; P.v_rad = {v + 3, vs};
        P.v_o = {filtered ? v + 4 : nullptr, vs}; P.v_vox = {filtered ? v + 5 : nullptr, vs};
    } else {
        HIP_CHECK(ctx->d_vd.reserve(nv)); HIP_CHECK(ctx->d_vthr.reserve(nv)); HIP_CHECK(ctx->d_vbsdf.reserve(nv)); HIP_CHECK(ctx->d_vrad.reserve(nv));
        if (filtered) { HIP_CHECK(ctx->d_vo.reserve(nv)); HIP_CHECK(ctx->d_vvox.reserve(nv)); }
        P.ray_o = {ctx->d_ray_o.p, 1}; P.ray_d = {ctx->d_ray_d.p, 1}; P.thr = {ctx->d_thr.p, 1}; P.li = {ctx->d_li.p, 1}; P.hit = {ctx->d_hit.p, 1};
        P.misc = {ctx->d_misc.p, 1};
        P.v_d = {ctx->d_vd.p, 1}; P.v_thr = {ctx->d_vthr.p, 1}; P.v_bsdf = {ctx->d_vbsdf.p, 1}; P.v_rad = {ctx->d_vrad.p, 1};
        P.v_o = {filtered ? ctx->d_vo.p : nullptr, 1}; P.v_vox = {filtered ? ctx->d_vvox.p : nullptr, 1};
    }
    P.nee_cos = nullptr;
    if (ctx->scene.env.w != 0 && ctx->nee != NEE_NEVER) { HIP_CHECK(ctx->d_neeCos.reserve(nn)); P.nee_cos = ctx->d_neeCos.p; }
    ctx->mediaArgs.path_medium = nullptr; ctx->mediaArgs.path_stride = 1;
    if (ctx->mediaArgs.media) { HIP_CHECK(ctx->d_pathMedium.reserve(nn)); ctx->mediaArgs.path_medium = ctx->d_pathMedium.p; }
    return PPG_OK;
}

// Buffers that otherwise grow with the first large round of the optimiser — the record arrays and the sort's — sized where the path state is
// sized (scene set-up), from the pass schedule an spp budget implies (renderSPP): a render then finds them in place instead of paying
// hipMalloc + first touch of a few GB in its second and third iteration (the first 20-pass render after a 5-pass warm-up ran 6 % below the
// later ones).  An estimate — 7 records per path plus max_vertices positions for every path k_tail may be handed —, not a limit: reserve()
// still grows what turns out too small.
int presizeRounds(ppg_ctx *ctx) {
    g_blockCache.prewarm();
    if (ctx->loss == LOSS_NONE || ctx->budgetType != 0 || !recordPositionsKnown(ctx->spatialFilter, false, ctx->nee)) return PPG_OK;  // (no iteration has sampled luminaires yet)
    const int nPasses = (int)std::ceil((size_t)ctx->budget / (float)ctx->sppPerPass);
    int rendered = 0, largest = 0;
    for (int it = 0; rendered < nPasses; ++it) {  // renderSPP, GP:1342-1426
        const int remaining = nPasses - rendered;
        int n = std::min(remaining, 1 << std::min(it, 30));
        if (remaining - n < 2 * n) n = remaining;
        if (n < remaining && it > 0) largest = std::max(largest, n);  // a training iteration with rounds (the first one has none: not built yet)
        rendered += n;
    }
    if (largest == 0) return PPG_OK;
    const size_t roundPaths = (size_t)ppg_adam_round_passes(ctx->sppPerPass, ctx->W, ctx->H, largest) * ctx->nPix * ctx->sppPerPass;
    const size_t handed = ctx->maxDepth < 0 ? std::min(roundPaths, std::max<size_t>(ctx->tailMin, roundPaths / ctx->tailDiv)) : 0;
    const size_t positions = std::min<size_t>(roundPaths * 7 + handed * (size_t)ctx->maxVertices, 0xfffffff0u);
    for (int k = 0; k < 2; ++k) { HIP_CHECK(ctx->d_adamKeys[k].reserve(positions)); HIP_CHECK(ctx->d_adamIdx[k].reserve(positions)); }
    HIP_CHECK(ctx->d_adamRecs.reserve(positions)); HIP_CHECK(ctx->d_splat.reserve(positions));
    HIP_CHECK(ctx->d_adamNv.reserve(roundPaths)); HIP_CHECK(ctx->d_adamBase.reserve(roundPaths));
    HIP_CHECK(ctx->d_nv8.reserve(roundPaths)); HIP_CHECK(ctx->d_straggler.reserve(roundPaths));
    if (handed) for (auto &g : ctx->strag) { HIP_CHECK(g.rec.reserve(handed * 8)); HIP_CHECK(g.orig.reserve(handed)); HIP_CHECK(g.count.reserve(2)); HIP_CHECK(g.ticket.reserve(1)); }
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, ctx->d_adamKeys[0].p, ctx->d_adamKeys[1].p, ctx->d_adamIdx[0].p, ctx->d_adamIdx[1].p, positions, 0u, 64u, ctx->stream));
        HIP_CHECK(ctx->d_sortTemp.reserve(std::max<size_t>(bytes, 16)));
    }
    return PPG_OK;
}

// stable LSD radix sort of the round's (key, record index) pairs on bits [beginBit, endBit); result in d_adamKeys[1] / d_adamIdx[1]
int sortAdamRecords(ppg_ctx *ctx, size_t n, unsigned int beginBit, unsigned int endBit) {
    hipStream_t s = ctx->stream;
    HIP_CHECK(ctx->d_adamKeys[1].reserve(n)); HIP_CHECK(ctx->d_adamIdx[1].reserve(n)); HIP_CHECK(ctx->d_adamIdx[0].reserve(n));
    if (ctx->adamIota < ctx->d_adamIdx[0].cap) {
        const unsigned int m = (unsigned int)ctx->d_adamIdx[0].cap;
        hipLaunchKernelGGL(k_iota, dim3((m + 255) / 256), dim3(256), 0, s, ctx->d_adamIdx[0].p, m);
        ctx->adamIota = m;
    }
    size_t bytes = 0;
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, ctx->d_adamKeys[0].p, ctx->d_adamKeys[1].p, ctx->d_adamIdx[0].p, ctx->d_adamIdx[1].p, n, beginBit, endBit, s));
    HIP_CHECK(ctx->d_sortTemp.reserve(std::max<size_t>(bytes, 16)));
    HIP_CHECK(rocprim::radix_sort_pairs((void *)ctx->d_sortTemp.p, bytes, ctx->d_adamKeys[0].p, ctx->d_adamKeys[1].p, ctx->d_adamIdx[0].p, ctx->d_adamIdx[1].p, n, beginBit, endBit, s));
    return PPG_OK;
}

// The deferred optimizeBsdfSamplingFraction calls of the round just rendered: sort by key, (multi-GPU: exchange through the round
// hook), apply leaf by leaf (k_adam_apply).  nRecords = positions used in d_adamKeys[0] / d_adamRecs (holes carry key ~0).
int applyAdamRound(ppg_ctx *ctx, size_t nRecords) {
    hipStream_t s = ctx->stream;
    const unsigned int nNodes = (unsigned int)ctx->snodes.size();
    if (nNodes >= (1u << 24)) { ctx->error = "S-tree exceeds 2^24 nodes with a bsdfSamplingFractionLoss"; return PPG_ERR_NOMEM; }
    unsigned int leafBits = 1;
    while ((1u << leafBits) <= nNodes) ++leafBits;  // every leaf index is below the all-ones pattern of a hole
    const unsigned int endBit = PPG_ADAM_LEAF_SHIFT + leafBits;
    if (ctx->sortedCommit && ctx->adamFlagShift != endBit) { ctx->error = "internal: flag bit of the round's records"; return PPG_ERR_STATE; }
    size_t n = nRecords;
    // The splats and the optimiser read the same sorted records and write different things (the building tree; the leaf headers' optimiser
    // state): k_splat_sorted runs on the second stream BESIDE the order / apply kernels — and beside the round hook's exchanges of a
    // sharded render —, whose serial chains leave most of the GPU idle.  Joined before the sorted arrays are reused and before returning.
    struct Join {
        ppg_ctx *c; bool forked = false;
        void now() { if (forked) { (void)hipStreamWaitEvent(c->stream, c->evJoin, 0); forked = false; } }
        ~Join() { now(); }
    } join{ctx};
    // (without a round hook the optimiser's kernels leave the context's stream too: ppg_ctx::treePending)
    const bool aside = ctx->sortedCommit && !ctx->passHook && sideStreamsAllowed(ctx) && !ctx->tuneNoAside;
    hipStream_t sa = aside ? ctx->stream3 : s;  // where the order / apply kernels go
    struct AsideGuard {  // an early return with kernels already on stream3: the event joinTree() waits for must lie behind them
        ppg_ctx *c; bool on;
        ~AsideGuard() { if (on && c->treePending) (void)hipEventRecord(c->evAdamDone, c->stream3); }
    } asideGuard{ctx, aside};
    if (n > 0) {
        int rc = PPG_OK;
        // (a round committed through records: one more bit, "a splat only", just above the leaf — those records sort behind the optimiser's)
        timedLaunch(ctx, "adam_sort(rocprim)", n, [&] { rc = sortAdamRecords(ctx, n, ctx->adamFast ? PPG_ADAM_LEAF_SHIFT : 0u, endBit + (ctx->sortedCommit ? 1u : 0u)); });
        if (rc) return rc;
        if (aside) {
            HIP_CHECK(hipEventRecord(ctx->evTreeFork, s));
            HIP_CHECK(hipStreamWaitEvent(ctx->stream2, ctx->evTreeFork, 0));
            HIP_CHECK(hipStreamWaitEvent(ctx->stream3, ctx->evTreeFork, 0));
            const unsigned int chunks = (unsigned int)((n + PPG_SPLAT_CHUNK - 1) / PPG_SPLAT_CHUNK);
            SplatLaunch a{(int)std::max(1u, std::min(chunks, 256u * 8u)), ctx->stream2, ctx->devTree(), ctx->d_adamKeys[1].p, ctx->d_adamIdx[1].p, ctx->d_splat.p, (unsigned int)n, leafBits, ctx->tuneSplatLdsNodes};
            ppg_launch_splat(ctx->directionalFilter, a);
            HIP_CHECK(hipEventRecord(ctx->evSplatDone, ctx->stream2));
            // (from here on work is in flight beside the context's stream: whatever happens below — an early return included — joinTree()
            // must wait for both side streams; the optimiser's event is recorded again behind its kernels)
            HIP_CHECK(hipEventRecord(ctx->evAdamDone, ctx->stream3));
            ctx->treePending = true;
            HIP_CHECK(hipGetLastError());
        } else if (ctx->sortedCommit) {  // DTree::recordIrradiance of every record of the round, D-tree by D-tree (ppg_kernels.h "The commit of a ROUND")
            const unsigned int chunks = (unsigned int)((n + PPG_SPLAT_CHUNK - 1) / PPG_SPLAT_CHUNK);
            SplatLaunch a{(int)std::max(1u, std::min(chunks, 256u * 8u)), s, ctx->devTree(), ctx->d_adamKeys[1].p, ctx->d_adamIdx[1].p, ctx->d_splat.p, (unsigned int)n, leafBits, ctx->tuneSplatLdsNodes};
            if (sideStreamsAllowed(ctx)) {
                HIP_CHECK(hipEventRecord(ctx->evFork, s));
                HIP_CHECK(hipStreamWaitEvent(ctx->stream2, ctx->evFork, 0));
                a.stream = ctx->stream2;
                ppg_launch_splat(ctx->directionalFilter, a);
                HIP_CHECK(hipEventRecord(ctx->evJoin, ctx->stream2));
                join.forked = true;
            } else timedLaunch(ctx, "k_splat_sorted", n, [&] { ppg_launch_splat(ctx->directionalFilter, a); });
            HIP_CHECK(hipGetLastError());
        }
    }
    if (ctx->passHook) {
        // hand the valid records over in key order, compact
        unsigned int nValid = 0;
        if (n > 0) {
            hipLaunchKernelGGL(k_count_valid, dim3(1), dim3(1), 0, s, ctx->d_adamKeys[1].p, (unsigned int)n, ctx->d_adamCount.p,
                               ctx->sortedCommit ? (1ull << ctx->adamFlagShift) : ~0ull);  // (the optimiser's records come first)
            HIP_CHECK(hipMemcpyAsync(&nValid, ctx->d_adamCount.p, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            HIP_CHECK(ctx->d_adamRecsOut.reserve(std::max<size_t>(1, nValid)));
            if (nValid) hipLaunchKernelGGL(k_gather_records, dim3((nValid + 255) / 256), dim3(256), 0, s, ctx->d_adamRecs.p, ctx->d_adamIdx[1].p, ctx->d_adamRecsOut.p, nValid);
        } else HIP_CHECK(ctx->d_adamRecsOut.reserve(1));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx->inHook = true; ctx->hookReplaced = false; ctx->hookCount = nValid; ctx->hookPhase = 0; ctx->ownerMode = false;
        const int hrc = ctx->passHook(ctx->passHookUser);
        ctx->inHook = false;
        if (hrc != 0) { ctx->error = "round hook failed"; return PPG_ERR_INVALID; }
        if (ctx->hookReplaced) {  // the union over all ranks, in d_adamRecs: sort it by the whole key
            join.now();  // (the sort below overwrites the arrays k_splat_sorted reads)
            n = (size_t)ctx->hookCount;
            if (n > 0) {
                HIP_CHECK(ctx->d_adamKeys[0].reserve(n));
                hipLaunchKernelGGL(k_record_keys, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, ctx->d_adamRecs.p, ctx->d_adamKeys[0].p, (unsigned int)n);
                int rc = sortAdamRecords(ctx, n, 0u, endBit);
                if (rc) return rc;
            }
        }
    }
    if (n > 0) {
        const unsigned int nl = (unsigned int)ctx->leaves.size();
        // One wave per D-tree walks its records as a serial chain, so the launch lasts as long as its busiest D-tree — if that one starts
        // last, everything else has finished by then: the D-trees are taken in descending order of their record counts.
        const unsigned int *order = nullptr;
        if (!ctx->tuneAdamUnordered && nl > 1) {
            for (int k = 0; k < 2; ++k) { HIP_CHECK(ctx->d_adamLeafCount[k].reserve(nl)); HIP_CHECK(ctx->d_adamLeafOrder[k].reserve(nl)); }
            size_t bytes = 0;
            HIP_CHECK(rocprim::radix_sort_pairs_desc(nullptr, bytes, ctx->d_adamLeafCount[0].p, ctx->d_adamLeafCount[1].p, ctx->d_adamLeafOrder[0].p, ctx->d_adamLeafOrder[1].p, (size_t)nl, 0u, 32u, sa));
            HIP_CHECK(ctx->d_orderTemp.reserve(std::max<size_t>(bytes, 16)));  // (its own scratch: the next batch's scans use d_sortTemp on the context's stream)
            timedLaunch(ctx, "adam_order", nl, [&] {
                hipLaunchKernelGGL(k_adam_counts, dim3((nl + 255u) / 256u), dim3(256), 0, sa, ctx->d_leaves.p, nl, ctx->d_adamKeys[1].p, (unsigned int)n, ctx->d_adamLeafCount[0].p,
                                   ctx->d_adamLeafOrder[0].p);
                (void)rocprim::radix_sort_pairs_desc((void *)ctx->d_orderTemp.p, bytes, ctx->d_adamLeafCount[0].p, ctx->d_adamLeafCount[1].p, ctx->d_adamLeafOrder[0].p,
                                                     ctx->d_adamLeafOrder[1].p, (size_t)nl, 0u, 32u, sa);
            });
            order = ctx->d_adamLeafOrder[1].p;
        }
        timedLaunch(ctx, "k_adam_apply", n, [&] {
            hipLaunchKernelGGL(k_adam_apply, dim3((nl * 64u + 255u) / 256u), dim3(256), 0, sa, ctx->d_hdr.p, ctx->d_leaves.p, order, nl, ctx->d_adamKeys[1].p, ctx->d_adamIdx[1].p,
                               ctx->d_adamRecs.p, (unsigned int)n, ctx->loss);
        });
        HIP_CHECK(hipGetLastError());
        if (aside) {
            HIP_CHECK(hipEventRecord(ctx->evAdamDone, ctx->stream3));
            ctx->treePending = true;
        }
    }
    if (ctx->passHook && ctx->ownerMode) {  // one owner per D-tree: the owners publish the state they computed
        HIP_CHECK(hipStreamSynchronize(s));
        ctx->inHook = true; ctx->hookPhase = 1;
        const int hrc = ctx->passHook(ctx->passHookUser);
        ctx->inHook = false; ctx->hookPhase = 0; ctx->ownerMode = false;
        if (hrc != 0) { ctx->error = "round hook failed"; return PPG_ERR_INVALID; }
    }
    return PPG_OK;
}

// ------------------------------------------------------------------------------------------------
// Stragglers
// ------------------------------------------------------------------------------------------------
// A guided path survives Russian roulette with probability 0.99 (GP:2124-2139): of the millions of paths of a batch a few hundred are still
// alive after 64 bounces and the longest runs for 300-900 — dependent bounces of ~12 us each, during which one wave works and the GPU waits
// (KITCHEN: 8 % of a 1023-pass render on one GPU, and the term that does not shrink when the image is sharded over eight).  So k_tail runs
// the handed-over paths only up to depth `deferDepth`; the STRAGGLERS — alive at that depth — are written to a compact set (path record by
// k_tail itself, vertex slots by k_extract_vertices), and a second k_tail finishes them on stream4 BESIDE the next batch's kernels, one path
// per wave.  What the batch still owes then — its film kernel (which needs the stragglers' radiance: the batch's Li values are kept in
// d_liKeep and the stragglers' scattered into it), the stragglers' commit — is done by the NEXT batch once its own tail has run
// (drainStragglers), or at the end of the ppg_render_passes call (flushStragglers).  The film sums keep their order and the building tree's
// sums are integers: for a batch without optimiser records nothing changes but the schedule.  In a round of the optimiser the stragglers'
// records are applied one round late — part of the result, the rule is in include/ppg.h ("STRAGGLERS") and in the oracle.
int addGroups(ppg_ctx *ctx, unsigned int first, unsigned int count);

// the compact state of n stragglers over the set's buffers (path records interleaved as k_tail wrote them; vertex slots [slot][path])
int stragglerState(ppg_ctx *ctx, ppg_ctx::Stragglers &G, const PathState &batch, unsigned int n, bool withVertices) {
    const bool filtered = ctx->spatialFilter != SF_NEAREST;
    const unsigned int vs = filtered ? 6u : 4u;
    if (withVertices) HIP_CHECK(G.vert.reserve((size_t)n * (size_t)ctx->maxVertices * vs));
    HIP_CHECK(G.nv8.reserve(n)); HIP_CHECK(G.base.reserve(n));
    if (batch.nee_cos) HIP_CHECK(G.neeCos.reserve(n));
    PathState &Ps = G.P;
    Ps = batch;  // n_pix, pixels: the batch's (adam_path_id)
    Ps.n_paths = n;
    float4 *r = G.rec.p, *v = G.vert.p;
    Ps.ray_o = {r, 8}; Ps.ray_d = {r + 1, 8}; Ps.thr = {r + 2, 8}; Ps.li = {r + 3, 8}; Ps.hit = {r + 4, 8}; Ps.misc = {reinterpret_cast<uint4 *>(r + 5), 8};
    Ps.v_d = {v, vs}; Ps.v_thr = {v + 1, vs}; Ps.v_bsdf = {v + 2, vs}; Ps.v_rad = {v + 3, vs};
    Ps.v_o = {filtered ? v + 4 : nullptr, vs}; Ps.v_vox = {filtered ? v + 5 : nullptr, vs};
    Ps.nee_cos = batch.nee_cos ? G.neeCos.p : nullptr;
    Ps.orig = G.orig.p;
    return PPG_OK;
}

// A batch on its way through renderBatch: what it works on, what planBatch decided about it, what has been counted so far.
struct Batch {
    PathState P, Pc;                // Pc: P with the contiguous copy of the path words, once copyMisc has made it
    DevScene S;
    MediaArgs M;                    // the media family's extra arguments
    HetArgs V;                      // the hetmedia family's
    DevTree T;
    RenderParams R;
    Queues Q;
    BatchPlan plan;
    int grid = 0, gridAll = 0;      // workgroups of the wavefront kernels / of a kernel over every path
    bool smallScene = false;
    size_t ldsBytes = 0;            // k_tail's dynamic LDS
    unsigned int *dense = nullptr;  // the live paths in one list (k_tail's work list)
    unsigned int hostCount = 0;     // live paths as far as the host knows (kernel timing wants the units of every launch)
    int bouncesRun = 0;
    bool miscCopied = false;
    size_t nRecordsOwn = 0, nRecords = 0;  // record positions of the round's own paths / with those of the previous round's stragglers
    unsigned int nStrag = 0;        // paths alive at the hand-over depth of a split tail
};

// variant of ppg_launch_tail
int tailVariant(const ppg_ctx *ctx) { return (isSmallScene(ctx) ? 4 : 0) | (ctx->doNee ? 2 : 0) | (ctx->fullMaterials ? 1 : 0); }

// The commit of a launch's vertices: in a round that commits through records (`records`) k_commit_records, else k_commit.
const char *commitName(bool records) { return records ? "k_commit_records" : "k_commit"; }
void launchCommitKernels(ppg_ctx *ctx, const CommitLaunch &a, bool records) {
    if (records) ppg_launch_commit_records(ctx->spatialFilter, a);
    else ppg_launch_commit(ctx->spatialFilter, ctx->directionalFilter, a);
}

// The record arrays of a round with n positions, every key a hole.  (The caller's DevTree is stale afterwards.)
int reserveRoundRecords(ppg_ctx *ctx, size_t n) {
    HIP_CHECK(ctx->d_adamKeys[0].reserve(std::max<size_t>(1, n))); HIP_CHECK(ctx->d_adamRecs.reserve(std::max<size_t>(1, n)));
    if (ctx->sortedCommit) HIP_CHECK(ctx->d_splat.reserve(std::max<size_t>(1, n)));
    if (n) HIP_CHECK(hipMemsetAsync(ctx->d_adamKeys[0].p, 0xff, n * 8, ctx->stream));
    return PPG_OK;
}

// After the first k_tail of a batch: B.nStrag paths wait in the current set.  Take their vertex slots and the batch's radiance, start their own
// k_tail (on stream4 when side streams are allowed), and leave the set pending.
int launchStragglers(ppg_ctx *ctx, const Batch &B) {
    hipStream_t s = ctx->stream;
    const PathState &P = B.P;
    const unsigned int nStrag = B.nStrag;
    const bool commit = B.plan.commit, beside = B.plan.beside;
    ppg_ctx::Stragglers &G = ctx->strag[ctx->stragCur];
    { int rc = stragglerState(ctx, G, P, nStrag, commit); if (rc) return rc; }
    G.n = nStrag; G.commit = commit; G.adam = B.plan.deferRecords && commit;
    const int small = gridFor(nStrag, 64, 1024);
    if (commit) hipLaunchKernelGGL(k_extract_vertices, dim3(small), dim3(256), 0, s, P, G.P, nStrag, (unsigned int)ctx->maxVertices);
    else if (P.nee_cos) hipLaunchKernelGGL(k_extract_nee_cos, dim3(small), dim3(256), 0, s, P, G.P, nStrag);  // (nothing recorded: a final iteration)
    HIP_CHECK(ctx->d_liKeep.reserve(P.n_paths));
    hipLaunchKernelGGL(k_copy_li, dim3(gridFor(P.n_paths)), dim3(256), 0, s, P, ctx->d_liKeep.p);
    if (G.iotaN < nStrag) {
        HIP_CHECK(G.iota.reserve(nStrag));
        const unsigned int m = (unsigned int)G.iota.cap;
        hipLaunchKernelGGL(k_iota, dim3((m + 255) / 256), dim3(256), 0, s, G.iota.p, m);
        G.iotaN = m;
    }
    HIP_CHECK(hipMemsetAsync(G.ticket.p, 0, 4, s));
    const TailShape shape = stragglerShape(nStrag);
    DevTree Tt = B.T;
    if (ctx->loss != LOSS_NONE && ctx->isBuilt) {  // the fractions of THIS round, whatever the optimiser does to the headers meanwhile
        const unsigned int nn = (unsigned int)ctx->snodes.size();
        HIP_CHECK(G.theta.reserve(nn));
        hipLaunchKernelGGL(k_copy_theta, dim3(gridFor(nn, 256, 256)), dim3(256), 0, s, ctx->d_hdr.p, nn, G.theta.p);
        Tt.theta_frozen = G.theta.p;
    }
    hipStream_t st = s;
    if (beside) {
        HIP_CHECK(hipEventRecord(ctx->evStragFork, s));
        HIP_CHECK(hipStreamWaitEvent(ctx->stream4, ctx->evStragFork, 0));
        st = ctx->stream4;
    }
    auto launch = [&] {
        RenderParams Rt = B.R;
        Rt.defer_depth = 0u;
        TailLaunch a{shape.grid, B.ldsBytes, st, G.P, B.S, Tt, Rt, G.iota.p, G.count.p, G.ticket.p, ctx->queues.stats, ctx->ldsTris,
                     ctx->d_tailLongest.p + (ctx->tailLaunches++ % PPG_TAIL_LOG), StragOut{nullptr, nullptr, nullptr}, shape.laneLimit, B.M, B.V};
        if (a.M.path_medium) { a.M.path_medium = reinterpret_cast<unsigned int *>(G.rec.p + 6); a.M.path_stride = 32; }  // (k_tail left the word in the record's seventh float4)
        ppg_launch_tail(tailVariant(ctx), a);
    };
    if (beside) { launch(); HIP_CHECK(hipEventRecord(ctx->evStragDone, ctx->stream4)); }
    else timedLaunch(ctx, "k_tail(stragglers)", nStrag, launch);  // (its own timer entry: in the product it runs beside the next batch, not on the critical path)
    G.pending = true; G.aside = beside;
    ctx->stragCur ^= 1;
    HIP_CHECK(hipGetLastError());
    return PPG_OK;
}

// What the previous batch still owes: its stragglers have ended (or the context's stream waits until they have) — their radiance into the
// kept copy, the batch's film kernel, their vertices' commit.  In a round of the optimiser their records take the positions from
// recordsFirst on of the round's arrays (sized for them by the caller).
int drainStragglers(ppg_ctx *ctx, size_t recordsFirst) {
    ppg_ctx::Stragglers &G = ctx->stragPrev();
    if (!G.pending) return PPG_OK;
    hipStream_t s = ctx->stream;
    if (G.aside) HIP_CHECK(hipStreamWaitEvent(s, ctx->evStragDone, 0));
    G.pending = false; G.aside = false;
    const int small = gridFor(G.n, 256, 1024);
    hipLaunchKernelGGL(k_scatter_li, dim3(small), dim3(256), 0, s, G.P, G.n, ctx->d_liKeep.p);
    if (G.film) { G.film(); G.film = nullptr; }
    if (G.commit) {
        hipLaunchKernelGGL(k_commit_prepare, dim3((G.n + 255) / 256), dim3(256), 0, s, G.P, (uint4 *)nullptr, G.nv8.p, (const unsigned char *)nullptr);
        DevTree T = ctx->devTree();
        const RenderParams R = ctx->params();
        if (G.adam) {
            if (!T.adam_keys) { ctx->error = "internal: stragglers' records outside a round"; return PPG_ERR_STATE; }
            // Record positions are key order within a D-tree (the round's sort is stable and looks at the leaf bits only): the stragglers take
            // theirs in the order of their paths' ids — k_tail handed them over in whatever order its waves got there.
            HIP_CHECK(G.origSorted.reserve(G.n)); HIP_CHECK(G.perm.reserve(G.n));
            size_t bytes = 0;
            HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, G.orig.p, G.origSorted.p, G.iota.p, G.perm.p, (size_t)G.n, 0u, 32u, s));
            HIP_CHECK(ctx->d_sortTemp.reserve(std::max<size_t>(bytes, 16)));
            HIP_CHECK(rocprim::radix_sort_pairs((void *)ctx->d_sortTemp.p, bytes, G.orig.p, G.origSorted.p, G.iota.p, G.perm.p, (size_t)G.n, 0u, 32u, s));
            hipLaunchKernelGGL(k_ranked_base, dim3(small), dim3(256), 0, s, G.base.p, G.perm.p, G.n, (unsigned int)recordsFirst, (unsigned int)ctx->maxVertices);
            T.adam_base = G.base.p;
        }
        CommitLaunch a{gridFor(G.n, 64, ctx->nBlocks), s, G.P, T, R, ctx->queues, G.nv8.p, nullptr, nullptr, ctx->d_splat.p, ctx->adamFlagShift};
        const bool records = G.adam && ctx->sortedCommit;
        timedLaunch(ctx, commitName(records), 0, [&] { launchCommitKernels(ctx, a, records); });
    }
    HIP_CHECK(hipGetLastError());
    return PPG_OK;
}

// End of a ppg_render_passes call: nothing may stay owed (the variance estimate reads the image, ppg_build_sdtree the building tree).  The
// records of the last round's stragglers are applied in a round of their own (include/ppg.h "STRAGGLERS"); `hookRound`: a sharded render's
// round hook is called for it on every rank, with or without records.
int flushStragglers(ppg_ctx *ctx, bool hookRound) {
    ppg_ctx::Stragglers &G = ctx->stragPrev();
    const bool records = G.pending && G.adam;
    if (!G.pending && !hookRound) return PPG_OK;
    ctx->joinTree();  // (the last round's splats and optimiser steps read the record arrays this round is about to overwrite)
    size_t n = 0;
    if (records || hookRound) {
        ctx->adamActive = true; ctx->adamFast = true;
        ctx->adamFlagShift = adamFlagShift(ctx->snodes.size());
        // (a few thousand vertices spread over all D-trees: k_commit's global atomics — k_splat_sorted would stage a D-tree in LDS for every
        // record or two, 5 ms for the 50 000 record positions of KITCHEN's 2-pass rounds; integer sums, the same bits)
        ctx->sortedCommit = false;
        n = records ? (size_t)G.n * (size_t)ctx->maxVertices : 0;
        int rc = reserveRoundRecords(ctx, n);
        if (rc) return rc;
    }
    int rc = drainStragglers(ctx, 0);
    if (!rc && (records || hookRound)) rc = applyAdamRound(ctx, n);
    ctx->adamActive = false;
    return rc;
}

// Filtered film (ppg_set_rfilter).  The footprint: zeroed at the start of every ppg_render_passes() call, then source pixels add their
// samples to it launch by launch (k_film_filter), and a resolve (k_film_resolve) moves it — zeroing it — into the call's image and the
// iteration's film at the end of the call, or into a final group's slot when the group is complete.
// Sharded by tiles, the footprint of a rank lacks what foreign source pixels within the filter's border of its tiles put on its targets:
// the BORDER SLOTS (include/ppg.h "Footprint hook"; forEachBorderSlot below gives their order).  prepareHalo builds their table when the
// shard, the film or the filter has changed; exchangeFootprint packs this rank's share into the halo buffer, has the hook all-reduce it,
// unpacks what this rank's targets need and resolves those targets only.
template <typename F> void forEachBorderSlot(int W, int H, int ts, int world, int B, F &&fn) {
    const int T = 2 * B + 1, tilesX = (W + ts - 1) / ts;
    std::vector<int> col((size_t)W), row((size_t)H);  // owner of pixel (x, y) = (row[y] + col[x]) % world
    for (int x = 0; x < W; ++x) col[(size_t)x] = (x / ts) % world;
    for (int y = 0; y < H; ++y) row[(size_t)y] = (int)(((long long)(y / ts) * tilesX) % world);
    for (int dy = -B; dy <= B; ++dy)
        for (int dx = -B; dx <= B; ++dx) {
            const unsigned int o = (unsigned int)((dy + B) * T + (dx + B));
            for (int y = std::max(0, -dy); y < std::min(H, H - dy); ++y)
                for (int x = std::max(0, -dx); x < std::min(W, W - dx); ++x) {
                    const int so = (row[(size_t)y] + col[(size_t)x]) % world, to = (row[(size_t)(y + dy)] + col[(size_t)(x + dx)]) % world;
                    if (so != to) fn(o, (unsigned int)y * (unsigned int)W + (unsigned int)x, so, to);
                }
        }
}
const char *kShardedMedia = "participating media are not supported in a sharded render (ppg_set_shard with world > 1): the scene binds a medium";
const char *kShardedFilter = "sharded filtered renders are not supported yet without a footprint hook: a reconstruction filter other than the default box "
                             "needs world = 1, or ppg_set_footprint_hook before the filter and the shard meet";
int prepareHalo(ppg_ctx *ctx) {
    const int key[6] = {ctx->W, ctx->H, ctx->tileSize, ctx->shardWorld, ctx->shardRank, ctx->rfBorder};
    if (memcmp(key, ctx->haloKey, sizeof key) != 0) {
        std::vector<unsigned int> src, pack, unpack;
        std::vector<unsigned char> tap;
        const int rank = ctx->shardRank;
        bool tooMany = false;
        forEachBorderSlot(ctx->W, ctx->H, ctx->tileSize, ctx->shardWorld, ctx->rfBorder, [&](unsigned int o, unsigned int s, int so, int to) {
            if (src.size() >= 0xffffffffu / 7u) { tooMany = true; return; }
            const unsigned int m = (unsigned int)src.size();
            src.push_back(s); tap.push_back((unsigned char)o);
            if (so == rank) pack.push_back(m);
            if (to == rank) unpack.push_back(m);
        });
        if (tooMany) { ctx->error = "sharded filtered film: too many border slots"; return PPG_ERR_NOMEM; }
        memset(ctx->haloKey, 0, sizeof ctx->haloKey);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (an earlier call's kernels may still read the old table)
        HIP_CHECK(ctx->d_haloSrc.reserve(std::max<size_t>(1, src.size())));
        HIP_CHECK(ctx->d_haloTap.reserve(std::max<size_t>(1, tap.size())));
        HIP_CHECK(ctx->d_haloPack.reserve(std::max<size_t>(1, pack.size())));
        HIP_CHECK(ctx->d_haloUnpack.reserve(std::max<size_t>(1, unpack.size())));
        HIP_CHECK(ctx->d_halo.reserve(std::max<size_t>(1, 7 * src.size())));
        if (!src.empty()) {
            HIP_CHECK(hipMemcpy(ctx->d_haloSrc.p, src.data(), src.size() * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(ctx->d_haloTap.p, tap.data(), tap.size(), hipMemcpyHostToDevice));
        }
        if (!pack.empty()) HIP_CHECK(hipMemcpy(ctx->d_haloPack.p, pack.data(), pack.size() * 4, hipMemcpyHostToDevice));
        if (!unpack.empty()) HIP_CHECK(hipMemcpy(ctx->d_haloUnpack.p, unpack.data(), unpack.size() * 4, hipMemcpyHostToDevice));
        ctx->haloM = (unsigned int)src.size(); ctx->haloPackN = (unsigned int)pack.size(); ctx->haloUnpackN = (unsigned int)unpack.size();
        memcpy(ctx->haloKey, key, sizeof key);
    }
    return PPG_OK;
}
int prepareFootprint(ppg_ctx *ctx) {
    const size_t T = 2 * (size_t)ctx->rfBorder + 1, floats = T * T * 7 * (size_t)ctx->W * (size_t)ctx->H;
    HIP_CHECK(ctx->d_foot.reserve(floats));
    HIP_CHECK(hipMemsetAsync(ctx->d_foot.p, 0, floats * 4, ctx->stream));
    ctx->rf.W = ctx->W; ctx->rf.H = ctx->H;
    if (ctx->exchangesFootprints()) return prepareHalo(ctx);
    return PPG_OK;
}
void launchFilmFilter(ppg_ctx *ctx, const PathState &P, unsigned long long seed, unsigned int base, unsigned int gs, unsigned int gstride, int j0, int j1) {
    timedLaunch(ctx, "k_film_filter", (uint64_t)P.n_pix * (uint64_t)(j1 - j0), [&] {
        const dim3 g((P.n_pix + 255) / 256), b(256);
        switch (ctx->rfBorder) {
        case 0: hipLaunchKernelGGL(k_film_filter<0>, g, b, 0, ctx->stream, P, ctx->rf, seed, base, gs, gstride, j0, j1, ctx->d_foot.p); break;
        case 1: hipLaunchKernelGGL(k_film_filter<1>, g, b, 0, ctx->stream, P, ctx->rf, seed, base, gs, gstride, j0, j1, ctx->d_foot.p); break;
        case 2: hipLaunchKernelGGL(k_film_filter<2>, g, b, 0, ctx->stream, P, ctx->rf, seed, base, gs, gstride, j0, j1, ctx->d_foot.p); break;
        default: hipLaunchKernelGGL(k_film_filter<3>, g, b, 0, ctx->stream, P, ctx->rf, seed, base, gs, gstride, j0, j1, ctx->d_foot.p); break;
        }
    });
}
void launchFilmResolve(ppg_ctx *ctx, float *im, float *sq, float *w, float *film, float *film_w) {
    const unsigned int n = (unsigned int)ctx->W * (unsigned int)ctx->H;
    timedLaunch(ctx, "k_film_resolve", n, [&] {
        const dim3 g((n + 255) / 256), b(256);
        switch (ctx->rfBorder) {
        case 0: hipLaunchKernelGGL(k_film_resolve<0>, g, b, 0, ctx->stream, ctx->rf, ctx->d_foot.p, im, sq, w, film, film_w); break;
        case 1: hipLaunchKernelGGL(k_film_resolve<1>, g, b, 0, ctx->stream, ctx->rf, ctx->d_foot.p, im, sq, w, film, film_w); break;
        case 2: hipLaunchKernelGGL(k_film_resolve<2>, g, b, 0, ctx->stream, ctx->rf, ctx->d_foot.p, im, sq, w, film, film_w); break;
        default: hipLaunchKernelGGL(k_film_resolve<3>, g, b, 0, ctx->stream, ctx->rf, ctx->d_foot.p, im, sq, w, film, film_w); break;
        }
    });
}
void launchFilmResolveOwned(ppg_ctx *ctx, float *im, float *sq, float *w, float *film, float *film_w) {
    const unsigned int n = ctx->nPix;
    if (!n) return;
    timedLaunch(ctx, "k_film_resolve_owned", n, [&] {
        const dim3 g((n + 255) / 256), b(256);
        switch (ctx->rfBorder) {
        case 0: hipLaunchKernelGGL(k_film_resolve_owned<0>, g, b, 0, ctx->stream, ctx->rf, ctx->d_pixels.p, n, ctx->d_foot.p, im, sq, w, film, film_w); break;
        case 1: hipLaunchKernelGGL(k_film_resolve_owned<1>, g, b, 0, ctx->stream, ctx->rf, ctx->d_pixels.p, n, ctx->d_foot.p, im, sq, w, film, film_w); break;
        case 2: hipLaunchKernelGGL(k_film_resolve_owned<2>, g, b, 0, ctx->stream, ctx->rf, ctx->d_pixels.p, n, ctx->d_foot.p, im, sq, w, film, film_w); break;
        default: hipLaunchKernelGGL(k_film_resolve_owned<3>, g, b, 0, ctx->stream, ctx->rf, ctx->d_pixels.p, n, ctx->d_foot.p, im, sq, w, film, film_w); break;
        }
    });
}
// One due call of the footprint hook.  localStatus != 0 (this rank was cancelled or failed): a zeroed buffer and the status, so that the
// peers, who are in this exchange, learn of it there.  Any failure — this rank's, or a peer's through the hook's return value — ends the
// call's exchanges on every rank alike (footFailed).
int callFootprintHook(ppg_ctx *ctx, int localStatus) {
    const uint64_t floats = 7ull * ctx->haloM;
    int sync = (int)hipStreamSynchronize(ctx->stream);  // the hook may read the buffer from the host, or work on a stream of its own
    if (sync != 0 && !localStatus) { (void)hipGetLastError(); localStatus = 1; }
    ++ctx->footDone;
    const int hrc = ctx->footHook(ctx->footHookUser, ctx->d_halo.p, floats, localStatus);
    if (hrc != 0 || localStatus) {
        ctx->footFailed = true;
        if (!localStatus || ctx->error.empty()) ctx->error = "footprint hook failed";
        return PPG_ERR_INVALID;
    }
    return PPG_OK;
}
// The footprint is complete on this rank's tiles: pack, hook, unpack, and resolve this rank's targets into im / sq / w (and film / film_w).
int exchangeFootprint(ppg_ctx *ctx, float *im, float *sq, float *w, float *film, float *film_w) {
    const size_t n = (size_t)ctx->W * (size_t)ctx->H;
    const unsigned int M = ctx->haloM;
    hipStream_t s = ctx->stream;
    HIP_CHECK(hipMemsetAsync(ctx->d_halo.p, 0, std::max<size_t>(1, 7 * (size_t)M) * 4, s));
    if (ctx->seesCancel()) { (void)callFootprintHook(ctx, 1); return PPG_ERR_CANCELLED; }
    if (ctx->haloPackN) timedLaunch(ctx, "k_halo_pack", ctx->haloPackN, [&] {
        hipLaunchKernelGGL(k_halo_pack, dim3((ctx->haloPackN + 255) / 256), dim3(256), 0, s, ctx->d_haloPack.p, ctx->haloPackN, ctx->d_haloSrc.p, ctx->d_haloTap.p, M, n,
                           ctx->d_foot.p, ctx->d_halo.p);
    });
    { int rc = callFootprintHook(ctx, 0); if (rc) return rc; }
    if (ctx->haloUnpackN) timedLaunch(ctx, "k_halo_unpack", ctx->haloUnpackN, [&] {
        hipLaunchKernelGGL(k_halo_unpack, dim3((ctx->haloUnpackN + 255) / 256), dim3(256), 0, s, ctx->d_haloUnpack.p, ctx->haloUnpackN, ctx->d_haloSrc.p, ctx->d_haloTap.p, M, n,
                           ctx->d_foot.p, ctx->d_halo.p);
    });
    launchFilmResolveOwned(ctx, im, sq, w, film, film_w);
    HIP_CHECK(hipGetLastError());
    return PPG_OK;
}

// ---- The stages of renderBatch, in the order they run.  What each may do was decided by planBatch (ppg_batch_plan.h): B.plan. ----

// 1. B.P is the batch's pixels and paths.  The plan, the context's round state, the slow round's buffers, the launch arguments.
int prepareBatch(ppg_ctx *ctx, Batch &B, int batch, bool adamRound, const GroupLaunch *gl, bool last) {
    const PathState &P = B.P;
    hipStream_t s = ctx->stream;
    const ppg_ctx::Stragglers &prev = ctx->stragPrev();
    BatchFacts f;
    f.paths = P.n_paths; f.maxDepth = ctx->maxDepth; f.isFinalIter = ctx->isFinalIter; f.adamRound = adamRound; f.last = last;
    f.spatialFilter = ctx->spatialFilter; f.nee = ctx->nee; f.doNee = ctx->doNee;
    f.timerOn = ctx->timer.enabled; f.tuneNoOverlap = ctx->tuneNoOverlap; f.tuneNoSortedCommit = ctx->tuneNoSortedCommit; f.tuneSplitDepth = ctx->tuneSplitDepth;
    f.tailThreshold = ctx->tailThreshold; f.tailMin = ctx->tailMin; f.tailDiv = ctx->tailDiv;
    f.deferDepthAdam = ctx->deferDepthAdam; f.streeNodes = ctx->snodes.size();
    f.prevPendingWithRecords = prev.pending && prev.adam; f.prevStragglers = prev.n; f.maxVertices = ctx->maxVertices;
    B.plan = planBatch(f);
    // (the round state that devTree(), applyAdamRound and drainStragglers read)
    ctx->adamActive = adamRound; ctx->adamFast = B.plan.adamFast; ctx->sortedCommit = B.plan.sortedCommit; ctx->adamFlagShift = B.plan.adamFlagShift;
    if (adamRound && !B.plan.adamFast) {  // record positions are handed out as the records are made: room for 48 per path, the device counts
        const size_t cap = std::max<size_t>((size_t)1 << 16, std::min<size_t>((size_t)48 * P.n_paths, 0xfffffff0u));
        HIP_CHECK(ctx->d_adamKeys[0].reserve(cap)); HIP_CHECK(ctx->d_adamRecs.reserve(cap));
        HIP_CHECK(hipMemsetAsync(ctx->d_adamCount.p, 0, 8, s));
    }
    B.S = ctx->scene;
    B.M = ctx->mediaArgs;
    B.V = ctx->hetArgs;
    B.T = ctx->devTree();
    RenderParams &R = B.R;
    R = ctx->params();
    R.spp = ctx->sppPerPass * batch;  // sample j of the batch has sample index pass_index * sppPerPass + j, j < spp * batch
    R.pass_index_spp = (unsigned int)ctx->passesRendered * (unsigned int)ctx->sppPerPass;
    if (gl) {
        R.pass_index_spp = gl->firstPass * (unsigned int)ctx->sppPerPass;
        R.group_samples = gl->groupPasses * (unsigned int)ctx->sppPerPass;
        R.group_stride = gl->stridePasses * (unsigned int)ctx->sppPerPass;
    }
    B.Q = ctx->queues;
    B.dense = B.Q.items[1];
    B.grid = wavefrontGrid(ctx->nBlocks, ctx->tuneBlocksSmall, ctx->tuneSmallPaths, P.n_paths, ctx->queues.cap);
    B.gridAll = gridFor(P.n_paths);
    B.smallScene = isSmallScene(ctx);
    B.ldsBytes = B.smallScene ? (size_t)ctx->ldsTris * 48 : (size_t)PPG_LDS_STACK * PPG_BLOCK * 4;
    B.hostCount = P.n_paths;
    B.Pc = P;
    return PPG_OK;
}

// 2. k_generate and the wavefront bounces (B.P.n_paths > 0).
// Bounce 1 works on all paths of the batch; every later bounce on the dense list of live paths that k_scan_counts + k_gather_slices
// rebuild from k_shade's output slices (ppg_kernels.h "Queues").  Bounded paths (maxDepth > 0) run maxDepth bounces.  Unbounded
// paths run wavefront bounces until fewer than `stopBelow` paths are alive and hand those to the persistent-thread tail (k_tail).
// Nothing is read back in between: the host launches as many bounces as the previous batch's survival curve says this batch needs
// (planBounces); the device raises a stop flag when the live count has fallen below the threshold, and the kernels of the
// bounces launched beyond that point return at once.  The host synchronises once per batch.
int runWavefront(ppg_ctx *ctx, Batch &B) {
    const PathState &P = B.P;
    const DevScene &S = B.S;
    Queues &Q = B.Q;
    hipStream_t s = ctx->stream;
    const int grid = B.grid;
    const bool smallScene = B.smallScene;
    // (small scenes go through k_trace too: tracing them inside k_generate / k_shade was measured slower, DESIGN.md "Tuning switches")
    const bool neeOn = ctx->doNee;  // m_doNee of this iteration (doNeeWithSpp, GP:1331-1340)
    const bool fullMats = ctx->fullMaterials;  // any BSDF beyond diffuse / two-sided diffuse / mirror: the FULL kernel variants
    const size_t triBytes = (size_t)ctx->scene.n_tris * 48;
    const size_t traceLds = smallScene ? B.ldsBytes : (size_t)PPG_TRACE_STACK * PPG_BLOCK * 4 + (PPG_BLOCK / 64) * sizeof(PairLds);  // k_trace: + a wave's pair scratch
    const unsigned int stopBelow = B.plan.stopBelow;
    int qin = QIN_FIRST;
    timedLaunch(ctx, "k_generate", P.n_paths, [&] { hipLaunchKernelGGL(k_generate, dim3(B.gridAll), dim3(PPG_BLOCK), 0, s, P, S, B.R, Q); });
    if (B.M.path_medium) hipLaunchKernelGGL(k_fill_u32, dim3(B.gridAll), dim3(PPG_BLOCK), 0, s, B.M.path_medium, P.n_paths, B.M.camera_medium);  // every path starts in the sensor's medium
    const int maxBounces = planBounces(ctx->survival, P.n_paths, stopBelow, ctx->maxDepth, ctx->tuneBulkBounces, ctx->bounceMargin, B.plan.adamFast, ctx->deferDepthAdam);
    const bool liveCount = ctx->timer.enabled;  // kernel timing wants the units of every launch
    unsigned int *counts = ctx->d_bounceCounts.p;  // [0..63] live paths after bounce b, [64] the stop flag
    HIP_CHECK(hipMemsetAsync(counts, 0, 72 * 4, s));
    Q.stop = counts + 64;
    Q.dense_n = ctx->d_total.p;
    for (int b = 0; b < maxBounces; ++b) {
        // (the first bounce — every path of the batch, camera rays — is sorted only for the sake of the split into material classes)
        const bool sortSlices = fullMats && (qin == QIN_DENSE || (Q.n_common && !neeOn && !ctx->tuneNoSortFirst)) && ctx->d_queueSorted.p;
        // k_trace sorts its own slice when it has traced it (sort_slice, ppg_kernels.h)
        unsigned int *const trSorted = sortSlices ? ctx->d_queueSorted.p : nullptr;
        unsigned char *const trKeys = sortSlices ? ctx->d_sortKeys.p : nullptr;
        timedLaunch(ctx, "k_trace", B.hostCount, [&] {
            TraceLaunch a{grid, traceLds, s, P, S, Q, qin, smallScene ? 0 : ctx->ldsNodes, ctx->ldsTris, trSorted, trKeys, smallScene, ctx->timer.enabled};
            launcher(ppg_path_kernels[sceneFamily(S, B.M, B.V)].trace)(a);
        });
        int shadeIn = sortSlices ? QIN_SORTED : qin;
        ctx->joinTree();  // (k_generate and the first k_trace ran beside the previous round's optimiser: k_shade needs its result)
        // FULL scene, sorted slice, no luminaire sampling: the common material classes first, in their own leaner kernel (MSET_COMMON)
        // (also for a scene with disks or cylinders, although this kernel is compiled without their code: it shades triangle hits of the
        // common classes only — sort_slice keeps every non-triangle hit out of them —, traces nothing and, without luminaire sampling,
        // never calls emitter_sample_direct, where a shape's em_info entry would be read as a triangle range.  A variant of it that
        // traces or samples emitters must go through the scene's family like the others: ppg_launch_shade / ppg_launch_tail.)
        const bool split = shadeIn == QIN_SORTED && Q.n_common && !neeOn;
        if (split) {
            timedLaunch(ctx, "k_shade<common>", B.hostCount, [&] {
                ShadeLaunch a{grid, 0, s, P, S, B.T, B.R, Q, QIN_SORTED_COMMON, smallScene ? 1 : 0, ctx->d_queueSorted.p, B.M, B.V};
                ppg_launch_shade_common(a);
            });
            shadeIn = QIN_SORTED_REST;
        }
        timedLaunch(ctx, neeOn ? "k_shade<nee>" : (fullMats ? (split ? "k_shade<rest>" : "k_shade<full>") : "k_shade"), B.hostCount, [&] {
            const int small = smallScene ? 1 : 0;
            // dynamic LDS: the staged triangles (luminaire sampling on a small scene) or the shadow rays' BVH stack columns
            const size_t neeBytes = smallScene ? triBytes : (size_t)PPG_LDS_STACK * PPG_BLOCK * 4;
            const size_t lds = (neeOn || ctx->scene.has_null) ? neeBytes : 0;
            const int variant = (neeOn ? 2 : 0) | (fullMats ? 1 : 0);
            ShadeLaunch a{grid, lds, s, P, S, B.T, B.R, Q, shadeIn, small, ctx->d_queueSorted.p, B.M, B.V};
            ppg_launch_shade(variant, a);
        });
        qin = QIN_DENSE;
        ++B.bouncesRun;
        hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, Q.count[0], ctx->d_offsets.p, (unsigned int)grid, ctx->d_total.p,
                           counts + std::min(b, 63), counts + 64, stopBelow);
        hipLaunchKernelGGL(k_gather_slices, dim3(grid), dim3(PPG_BLOCK), 0, s, Q.items[0], Q.count[0], ctx->d_offsets.p, Q.cap, Q.items[1]);
        if (liveCount) {
            HIP_CHECK(hipMemcpyAsync(&B.hostCount, ctx->d_total.p, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (B.hostCount == 0 || (ctx->maxDepth < 0 && B.hostCount < stopBelow)) break;
        }
    }
    return PPG_OK;
}

// k_tail over the dense list, up to `depth` (0: every path to its end).  handedPaths: how many paths it will find, when the host knows — 0 = unknown.
int launchTail(ppg_ctx *ctx, Batch &B, unsigned int depth, size_t handedPaths) {
    hipStream_t s = ctx->stream;
    ppg_ctx::Stragglers &G = ctx->strag[ctx->stragCur];  // the set this batch's stragglers go to (the other one may be pending: the previous batch's)
    HIP_CHECK(hipMemsetAsync(ctx->d_ticket.p, 0, 4, s));
    const TailShape shape = tailShape(B.grid, ctx->tuneTailBlocks, handedPaths);
    timedLaunch(ctx, "k_tail", B.hostCount, [&] {
        RenderParams Rt = B.R;
        Rt.defer_depth = depth;
        // (the launch's longest path is logged for launches that run their paths to the END: the sum is the tails' critical path; a launch that
        // hands its stragglers over writes to a spare slot nobody reads)
        TailLaunch a{shape.grid, B.ldsBytes, s, B.P, B.S, B.T, Rt, B.dense, ctx->d_total.p, ctx->d_ticket.p, B.Q.stats, ctx->ldsTris,
                     ctx->d_tailLongest.p + (depth ? PPG_TAIL_LOG : (ctx->tailLaunches++ % PPG_TAIL_LOG)), StragOut{G.rec.p, G.orig.p, G.count.p}, shape.laneLimit, B.M, B.V};
        ppg_launch_tail(tailVariant(ctx), a);
    });
    return PPG_OK;
}

// k_commit_prepare: a byte per path for k_commit's work items (+ the contiguous copy of the path words: with interleaved path records k_commit
// and k_path_nv would sweep the per-path word once per (slot, path) item)
int copyMisc(ppg_ctx *ctx, Batch &B) {
    const PathState &P = B.P;
    if (B.miscCopied || P.n_paths == 0) return PPG_OK;
    HIP_CHECK(ctx->d_nv8.reserve(P.n_paths));
    hipLaunchKernelGGL(k_commit_prepare, dim3((P.n_paths + 255) / 256), dim3(256), 0, ctx->stream, P, ctx->aosPaths ? ctx->d_miscCompact.p : (uint4 *)nullptr, ctx->d_nv8.p,
                       B.plan.overlap ? (const unsigned char *)ctx->d_straggler.p : (const unsigned char *)nullptr);
    if (ctx->aosPaths) B.Pc.misc = {ctx->d_miscCompact.p, 1};
    B.miscCopied = true;
    return PPG_OK;
}

// The batch's commit on stream st.  Ended: copyMisc left the stragglers' bytes 0; List: by list position, the bytes written just before.
void launchCommit(ppg_ctx *ctx, const Batch &B, hipStream_t st, CommitSet set) {
    const bool list = set == CommitSet::List;
    if (list) hipLaunchKernelGGL(k_commit_prepare_list, dim3(std::max(1, std::min(B.grid, 1024))), dim3(256), 0, st, B.P, B.dense, ctx->d_total.p, ctx->d_nv8.p);
    // (the stragglers' words changed in the tail: the list's paths are read in place)
    CommitLaunch a{B.grid, st, list ? B.P : B.Pc, B.T, B.R, B.Q, ctx->d_nv8.p, list ? B.dense : nullptr, list ? ctx->d_total.p : nullptr, ctx->d_splat.p, ctx->adamFlagShift};
    launchCommitKernels(ctx, a, ctx->sortedCommit);
}
// ... on the context's stream, with its timer entry (kernel timing is on only where side streams are not allowed)
void launchCommitTimed(ppg_ctx *ctx, const Batch &B, CommitSet set, uint64_t units) {
    timedLaunch(ctx, commitName(ctx->sortedCommit), units, [&] { launchCommit(ctx, B, ctx->stream, set); });
}

// k_tail, and with plan.overlap the commit of the paths that have ENDED when it takes over: beside it on stream2 — forked before the tail's
// launch, joined behind it —, or after it where side streams are not allowed.
int launchTailAndEndedCommit(ppg_ctx *ctx, Batch &B, unsigned int depth, size_t handedPaths) {
    hipStream_t s = ctx->stream;
    if (B.plan.overlap) HIP_CHECK(hipEventRecord(ctx->evFork, s));
    { int rc = launchTail(ctx, B, depth, handedPaths); if (rc) return rc; }
    if (!B.plan.overlap) return PPG_OK;
    if (B.plan.beside) {
        HIP_CHECK(hipStreamWaitEvent(ctx->stream2, ctx->evFork, 0));
        launchCommit(ctx, B, ctx->stream2, CommitSet::Ended);
        HIP_CHECK(hipEventRecord(ctx->evJoin, ctx->stream2));
        HIP_CHECK(hipStreamWaitEvent(s, ctx->evJoin, 0));
    } else launchCommitTimed(ctx, B, CommitSet::Ended, B.P.n_paths);
    return PPG_OK;
}

// 3. What follows the wavefront bounces of a batch (the shapes by plan: DESIGN.md "Launch structure on MI355X"):
//   unbounded paths   persistent threads finish the survivors (k_tail): ONE launch, every lane carries a path from the dense list until it
//                     ends.  Its length is set by the batch's LONGEST path (KITCHEN: 300-900 dependent bounces among 1-12 M paths); the
//                     crowd of short paths dies away around it and the wave that holds it speeds up as it empties;
//   training batches  k_commit splats every recorded vertex into the building tree.
// With both, k_commit for the paths that HAVE ended runs on a second stream beside k_tail, and a second, small k_commit takes the
// stragglers afterwards.  Integer accumulation makes the split invisible in the result.  In a round of the optimiser, the record
// positions must then be known before the tail has run: a straggler reserves max_vertices positions (unused ones stay holes).
// A split tail hands the paths still alive at plan.deferDepth over to a second launch that runs beside the NEXT batch ("Stragglers").
int finishPaths(ppg_ctx *ctx, Batch &B) {
    const PathState &P = B.P;
    const BatchPlan &plan = B.plan;
    hipStream_t s = ctx->stream;
    RoundReadback *const h = ctx->h_round;
    ctx->joinTree();  // (a batch without a wavefront bounce)
    if (plan.tail) {
        if (B.bouncesRun == 0)  // no wavefront bounce was run: every path of the batch goes to the persistent threads
            hipLaunchKernelGGL(k_iota_total, dim3(B.gridAll), dim3(PPG_BLOCK), 0, s, B.dense, P.n_paths, ctx->d_total.p);
        if (plan.overlap) {
            HIP_CHECK(ctx->d_straggler.reserve(P.n_paths));
            HIP_CHECK(hipMemsetAsync(ctx->d_straggler.p, 0, P.n_paths, s));
            hipLaunchKernelGGL(k_mark_list, dim3(B.grid), dim3(PPG_BLOCK), 0, s, B.dense, ctx->d_total.p, ctx->d_straggler.p);
        } else if (!plan.splitTail) {
            int rc = launchTail(ctx, B, 0u, 0);
            if (rc) return rc;
        }
    }
    if (plan.fastRound) {
        // position of path i's records = exclusive scan of the vertex counts
        HIP_CHECK(ctx->d_adamNv.reserve(P.n_paths)); HIP_CHECK(ctx->d_adamBase.reserve(P.n_paths));
        { int rc = copyMisc(ctx, B); if (rc) return rc; }
        hipLaunchKernelGGL(k_path_nv, dim3((P.n_paths + 255) / 256), dim3(256), 0, s, B.Pc, ctx->d_adamNv.p, plan.overlap ? ctx->d_straggler.p : nullptr, (unsigned int)ctx->maxVertices);
        size_t bytes = 0;
        HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, ctx->d_adamNv.p, ctx->d_adamBase.p, 0u, (size_t)P.n_paths, rocprim::plus<unsigned int>(), s));
        HIP_CHECK(ctx->d_sortTemp.reserve(std::max<size_t>(bytes, 16)));
        HIP_CHECK(rocprim::exclusive_scan((void *)ctx->d_sortTemp.p, bytes, ctx->d_adamNv.p, ctx->d_adamBase.p, 0u, (size_t)P.n_paths, rocprim::plus<unsigned int>(), s));
        HIP_CHECK(hipMemcpyAsync(&h->sumBase, ctx->d_adamBase.p + (P.n_paths - 1), 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&h->lastNv, ctx->d_adamNv.p + (P.n_paths - 1), 4, hipMemcpyDeviceToHost, s));
    }
    if (plan.tail || plan.fastRound) {
        if (plan.tail) HIP_CHECK(hipMemcpyAsync(h->live, ctx->d_bounceCounts.p, sizeof h->live, hipMemcpyDeviceToHost, s));
        if (plan.splitTail) HIP_CHECK(hipMemcpyAsync(&h->handed, ctx->d_total.p, 8, hipMemcpyDeviceToHost, s));  // the paths handed to k_tail
        HIP_CHECK(hipStreamSynchronize(s));  // the one host round trip of a batch of unbounded paths / of a round
        if (plan.tail) {
            // the survival curve of this batch sizes the schedule of the next one
            const int ran = observeBounces(ctx->survival, h->live, B.bouncesRun, P.n_paths, plan.stopBelow);
            if (ctx->debugBatch) {
                fprintf(stderr, "[ppg batch] iter %d paths %u built %d final %d launched %d ran %d stop<%u live:", ctx->iter, P.n_paths, (int)ctx->isBuilt, (int)ctx->isFinalIter, B.bouncesRun, ran, plan.stopBelow);
                for (int b = 0; b < ran; ++b) fprintf(stderr, " %u", h->live[b]);
                fprintf(stderr, "\n");
            }
        }
        if (plan.fastRound) {
            B.nRecordsOwn = (size_t)h->sumBase + h->lastNv;
            if (B.nRecordsOwn + plan.nDeferredIn > 0xfffffff0ull) { ctx->error = "too many Adam records in one round"; return PPG_ERR_NOMEM; }
        }
    }
    // (without paths of its own — a cancelled rank kept in step — a round may still owe the previous round's stragglers)
    if (plan.fastRound || (plan.adamFast && plan.nDeferredIn)) {
        B.nRecords = B.nRecordsOwn + plan.nDeferredIn;
        int rc = reserveRoundRecords(ctx, B.nRecords);
        if (rc) return rc;
        B.T = ctx->devTree();
    }
    if (plan.commit) { int rc = copyMisc(ctx, B); if (rc) return rc; }
    if (plan.splitTail) {
        // k_tail up to depth deferDepth; what is alive then is written to the straggler set (at most every path handed over)
        ppg_ctx::Stragglers &G = ctx->strag[ctx->stragCur];
        const size_t handed = (size_t)h->handed;
        HIP_CHECK(G.rec.reserve(std::max<size_t>(1, handed) * 8)); HIP_CHECK(G.orig.reserve(std::max<size_t>(1, handed)));
        HIP_CHECK(G.count.reserve(2)); HIP_CHECK(G.ticket.reserve(1));
        HIP_CHECK(hipMemsetAsync(G.count.p, 0, 16, s));
        { int rc = launchTailAndEndedCommit(ctx, B, plan.deferDepth, handed); if (rc) return rc; }
        HIP_CHECK(hipMemcpyAsync(&h->stragglers, G.count.p, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));  // the second host round trip of a batch with a split tail: how many stragglers
        B.nStrag = (unsigned int)h->stragglers;
        if (ctx->debugBatch) fprintf(stderr, "[ppg batch] iter %d stragglers %u of %zu handed over at depth %u\n", ctx->iter, B.nStrag, handed, plan.deferDepth);
        if (B.nStrag) {
            // (the previous batch's set is consumed before this batch's stragglers start: one event, one kept copy of the radiance)
            int rc = drainStragglers(ctx, B.nRecordsOwn);
            if (!rc) rc = launchStragglers(ctx, B);
            if (rc) return rc;
        }
        if (plan.overlap) launchCommitTimed(ctx, B, CommitSet::List, 0);
    } else if (plan.overlap) {
        int rc = launchTailAndEndedCommit(ctx, B, 0u, 0);
        if (rc) return rc;
        launchCommitTimed(ctx, B, CommitSet::List, 0);
    } else if (plan.commit) launchCommitTimed(ctx, B, CommitSet::All, P.n_paths);
    // what an earlier batch still owes (its film kernel, its stragglers' commit) comes before this batch's own sort and film kernel
    if (!B.nStrag) return drainStragglers(ctx, B.nRecordsOwn);  // (a batch with stragglers of its own consumed it above)
    return PPG_OK;
}

// 4. The round of the optimiser: its records are counted — a slow round's by the device —, sorted and applied.
int optimiserRound(ppg_ctx *ctx, Batch &B) {
    if (!ctx->adamFast) {
        RoundReadback *const h = ctx->h_round;
        HIP_CHECK(hipMemcpyAsync(&h->slowCount, ctx->d_adamCount.p, 8, hipMemcpyDeviceToHost, ctx->stream));  // (and slowOverflow)
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (h->slowOverflow) { ctx->error = "Adam record buffer overflow (box spatial filter / next-event estimation with a bsdfSamplingFractionLoss)"; return PPG_ERR_NOMEM; }
        B.nRecords = h->slowCount;
    }
    const int rc = applyAdamRound(ctx, B.nRecords);
    ctx->adamActive = false;
    return rc;
}

// 5. The batch's film kernel — at once, or, when stragglers of this batch are still running, from the copy of its paths' radiance once
// they have ended (drainStragglers): the sums a pixel's samples go through are the same either way.
void filmOrDefer(ppg_ctx *ctx, const Batch &B, int batch, const GroupLaunch *gl) {
    PathState Pf = B.P;
    const bool defer = B.nStrag > 0;
    if (defer) Pf.li = {ctx->d_liKeep.p, 1};
    const int sppBatch = ctx->sppPerPass * batch;
    const bool hasGl = gl != nullptr;
    const GroupLaunch glv = gl ? *gl : GroupLaunch{};
    const unsigned long long seed = B.R.seed;
    const unsigned int base = B.R.pass_index_spp, gs = B.R.group_samples, gstride = B.R.group_stride;
    auto film = [ctx, Pf, sppBatch, hasGl, glv, seed, base, gs, gstride] {
        hipStream_t st = ctx->stream;
        if (ctx->filtered) {  // footprint partials; a final launch's groups one by one, each resolved into its slot once it is complete
            if (!hasGl) launchFilmFilter(ctx, Pf, seed, base, 0u, 0u, 0, sppBatch);
            else {
                const size_t n = ctx->nPixAll;
                for (int j0 = 0, k = 0; j0 < sppBatch; j0 += (int)gs, ++k) {
                    launchFilmFilter(ctx, Pf, seed, base, gs, gstride, j0, std::min(sppBatch, j0 + (int)gs));
                    if (!glv.groupsDone || glv.exchange) continue;
                    float *slot = ctx->d_partials.p + (ctx->shardWorld > 1 ? 4 * n : 0) + (size_t)(glv.slot0 + (unsigned int)k * glv.slotStride) * 7u * n;
                    launchFilmResolve(ctx, slot, slot + 3 * n, slot + 6 * n, nullptr, nullptr);
                }
            }
            if (hasGl && glv.addCount) (void)addGroups(ctx, 0, glv.addCount);
            return;
        }
        timedLaunch(ctx, "k_film", Pf.n_pix, [&] {
            if (hasGl) hipLaunchKernelGGL(k_film_groups, dim3((Pf.n_pix + 255) / 256), dim3(256), 0, st, Pf, sppBatch, glv.groupPasses * (unsigned int)ctx->sppPerPass,
                                          ctx->d_partials.p + (ctx->shardWorld > 1 ? 4 * (size_t)ctx->nPixAll : 0), glv.slot0, glv.slotStride, ctx->nPixAll);
            else hipLaunchKernelGGL(k_film, dim3((Pf.n_pix + 255) / 256), dim3(256), 0, st, Pf, sppBatch, ctx->d_image.p, ctx->d_sq.p, ctx->d_imageW.p,
                                    ctx->d_film.p, ctx->d_filmW.p);
        });
        if (hasGl && glv.addCount) (void)addGroups(ctx, 0, glv.addCount);
    };
    if (defer) ctx->stragPrev().film = film; else film();  // (launchStragglers made this batch's set the previous one)
}


// `batch` BlockedRenderProcesses (GP:1087-1106 / renderBlock GP:1587-1641) over all owned pixels in one set of launches.
// adamRound: this batch is one round of the sampling-fraction optimiser.
// A launch of whole groups of a final iteration's passes (include/ppg.h "Final iteration: groups of passes"): `batch` passes = groups of
// groupPasses passes (the last one may be shorter; or a part of ONE group when groupPasses >= batch), the first starting at pass
// firstPass of the render, consecutive groups of the launch stridePasses apart; group k accumulates into slot slot0 + k * slotStride.
int renderBatch(ppg_ctx *ctx, int batch, bool adamRound, const GroupLaunch *gl = nullptr, bool last = true, const unsigned int *regionPixels = nullptr,
                unsigned int regionCount = 0) {
    Batch B{};
    PathState &P = B.P;
    P = ctx->paths;
    if (regionPixels) { P.n_pix = regionCount; P.pixels = regionPixels; }  // a round over ONE group of blocks (include/ppg.h "Rounds by image region")
    if (gl && gl->wholeFilm && ctx->shardWorld > 1) { P.n_pix = ctx->nPixAll; P.pixels = ctx->d_pixelsAll.p; }  // the whole film, not this rank's tiles
    P.n_paths = (unsigned int)((size_t)P.n_pix * ctx->sppPerPass * (size_t)batch);
    if (P.n_paths == 0 && !(adamRound && ctx->passHook)) return PPG_OK;
    int rc = prepareBatch(ctx, B, batch, adamRound, gl, last);
    if (!rc && P.n_paths > 0) rc = runWavefront(ctx, B);
    if (!rc) rc = finishPaths(ctx, B);
    if (!rc && adamRound) rc = optimiserRound(ctx, B);
    if (rc) return rc;
    if (P.n_paths > 0) filmOrDefer(ctx, B, batch, gl);
    HIP_CHECK(hipGetLastError());
    return PPG_OK;
}


// The passes of a FINAL iteration (spp budget), include/ppg.h "Final iteration: groups of passes": groups of ppg_final_group_passes(numPasses)
// passes, each summed on its own (k_film_groups) and added to image / film in group order (k_add_groups).  One GPU renders them all, several
// groups per launch; rank r of a sharded render renders groups r, r + world, ... over the WHOLE film — nothing is recorded in a final
// iteration (GP:2150-2154) and the sampler is keyed by (pixel, sample index), so the groups are independent, and a rank then pays 1 / world of
// the iteration's tails instead of all of them on its tiles — and leaves its slots for the exchange (ppg_final_partials).
int addGroups(ppg_ctx *ctx, unsigned int first, unsigned int count) {
    const unsigned int n = ctx->nPixAll;
    hipLaunchKernelGGL(k_add_groups, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, ctx->d_partials.p + (ctx->shardWorld > 1 ? 4 * (size_t)n : 0), first, count,
                       ctx->d_image.p, ctx->d_sq.p, ctx->d_imageW.p, ctx->d_film.p, ctx->d_filmW.p);
    return PPG_OK;
}
// How the groups of a sharded final iteration are dealt (include/ppg.h "Final iteration: groups of passes"): whole groups to the ranks when
// there are at least two per rank, otherwise every group to every rank ON ITS TILES — a 13-pass final iteration is ONE group, which one rank
// would render alone.  The sums a pixel's samples go through are the same either way (a group's partial per pixel, the partials in group
// order), so the picture does not depend on the choice.
static bool finalGroupsByRank(unsigned int nGroups, unsigned int world) { return world > 1 && nGroups >= 2u * world; }

int renderFinalGroups(ppg_ctx *ctx, int numPasses) {
    const unsigned int G = (unsigned int)ppg_final_group_passes(numPasses), nGroups = ((unsigned int)numPasses + G - 1) / G;
    const unsigned int world = (unsigned int)ctx->shardWorld, rank = (unsigned int)ctx->shardRank;
    const bool byRank = finalGroupsByRank(nGroups, world);  // else: all groups, this rank's tiles (world == 1: the whole film)
    const size_t n = ctx->nPixAll;
    std::vector<unsigned int> mine;
    for (unsigned int g = byRank ? rank : 0u; g < nGroups; g += byRank ? world : 1u) mine.push_back(g);
    auto passesOf = [&](unsigned int g) { return std::min(G, (unsigned int)numPasses - g * G); };
    // Passes per launch: maxBatchFinal.  PPG_FINAL_HALVES=1: when this rank's share of the iteration would fit ONE launch, half of it, so that the
    // stragglers of the first half finish beside the second half's paths ("Stragglers") — measured and NOT the default: each half hands its own
    // 2 M paths to k_tail (the floor below which wavefront bounces no longer fill the GPU), and that crowd phase, 10-12 ms of throughput on
    // KITCHEN, is then paid twice to hide 4 ms of a lone path (driver's command: 146 vs 154 Msamples/s, profiles/r06_experiments.json).  How the
    // passes are cut into launches does not enter any sum (a group's samples are added to its slot in sample order, launch after launch).
    unsigned int launchPasses = (unsigned int)ctx->maxBatchFinal;
    {
        unsigned int minePasses = 0;
        for (unsigned int g : mine) minePasses += passesOf(g);
        const size_t pixels = byRank || world == 1 ? n : (size_t)ctx->nPix;
        if (ctx->tuneFinalHalves && ctx->maxDepth < 0 && ctx->tuneSplitDepth > 0 && sideStreamsAllowed(ctx) && minePasses >= 2 && minePasses <= launchPasses &&
            pixels * (size_t)ctx->sppPerPass * (size_t)(minePasses / 2) >= ((size_t)1 << 21)) {
            launchPasses = (minePasses + 1) / 2;
            if (G < launchPasses) launchPasses = std::max(G, launchPasses / G * G);  // whole groups per launch
        }
    }
    // A filtered film rendered by tiles (include/ppg.h "Footprint hook"): one group at a time — its stragglers flushed, so that its footprint
    // is complete, then the borders exchanged and this rank's targets resolved into the group's slot.
    const bool exch = ctx->exchangesFootprints() && !byRank;
    auto exchangeGroup = [&](unsigned int g) -> int {
        int rc = flushStragglers(ctx, false);
        if (rc) return rc;
        float *slot = ctx->d_partials.p + 4 * n + (size_t)g * 7u * n;
        return exchangeFootprint(ctx, slot, slot + 3 * n, slot + 6 * n, nullptr, nullptr);
    };
    const unsigned int perLaunch = exch ? 1u : std::max(1u, launchPasses / G);  // whole groups per launch (G <= launchPasses), else parts of one group
    const unsigned int slots = world > 1 ? nGroups : std::max(perLaunch, std::max(1u, (unsigned int)ctx->maxBatchFinal / G));
    const size_t floats = (world > 1 ? 4 * n : 0) + (size_t)slots * 7 * n;
    if (ctx->d_partials.cap < floats || ctx->partialSlots != slots) {
        HIP_CHECK(ctx->d_partials.reserve(floats));
        ctx->partialSlots = slots;
    }
    HIP_CHECK(hipMemsetAsync(ctx->d_partials.p, 0, floats * 4, ctx->stream));
    const unsigned int firstPassAbs = (unsigned int)ctx->passesRendered;
    const unsigned int step = byRank ? world : 1u;  // distance between this rank's consecutive groups
    const uint64_t pixelsMine = byRank || world == 1 ? (uint64_t)n : (uint64_t)ctx->nPix;
    bool stop = false;
    for (size_t m = 0; m < mine.size() && !stop;) {
        if (ctx->seesCancel()) break;
        if (G <= launchPasses) {
            const size_t cnt = std::min<size_t>(perLaunch, mine.size() - m);
            unsigned int batch = 0;
            for (size_t q = 0; q < cnt; ++q) batch += passesOf(mine[m + q]);
            // (one GPU: the launch's slots are added to image and film right behind its film kernel)
            GroupLaunch gl{firstPassAbs + mine[m] * G, G, step * G, world > 1 ? mine[m] : 0u, world > 1 ? step : 1u, byRank, world == 1 ? (unsigned int)cnt : 0u};
            gl.exchange = exch;
            int rc = renderBatch(ctx, (int)batch, false, &gl, m + cnt >= mine.size());
            if (rc) return rc;
            ctx->samplesLocal += pixelsMine * batch * ctx->sppPerPass;
            if (exch && (rc = exchangeGroup(mine[m]))) return rc;
            m += cnt;
        } else {  // a group larger than a launch: its parts accumulate into the same slot one after the other
            const unsigned int g = mine[m], total = passesOf(g);
            for (unsigned int done = 0; done < total;) {
                if (ctx->seesCancel()) { stop = true; break; }
                const unsigned int batch = std::min(launchPasses, total - done);
                const bool lastPart = done + batch >= total;
                GroupLaunch gl{firstPassAbs + g * G + done, batch, batch, world > 1 ? g : 0u, 1u, byRank, (world == 1 && lastPart) ? 1u : 0u, lastPart};
                gl.exchange = exch;
                int rc = renderBatch(ctx, (int)batch, false, &gl, lastPart && m + 1 >= mine.size());
                if (rc) return rc;
                ctx->samplesLocal += pixelsMine * batch * ctx->sppPerPass;
                done += batch;
            }
            if (exch && !stop) { int rc = exchangeGroup(g); if (rc) return rc; }
            ++m;
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));  // bound the launch queue; lets ppg_cancel() take effect
    }
    { int rc = flushStragglers(ctx, false); if (rc) return rc; }
    ctx->passesRendered += numPasses; ctx->passesRenderedThisIter += numPasses; ctx->passesLocal += numPasses;
    if (world > 1) { ctx->partialsPending = true; ctx->pendingGroups = nGroups; }
    return ctx->seesCancel() ? PPG_ERR_CANCELLED : PPG_OK;
}

// The owned pixels grouped by region: region of a pixel = spiral rank of its 32x32 block * regions / blocks (include/ppg.h "Rounds by image
// region"); inside a group in the order of the owned-pixel list (row-major), so that a wave is still 64 neighbouring pixels of a row.
int buildRegionLists(ppg_ctx *ctx, int regions) {
    if (ctx->regionsBuilt == regions) return PPG_OK;
    const int bs = 32, bx = (ctx->W + bs - 1) / bs, by = (ctx->H + bs - 1) / bs;
    std::vector<int> rank((size_t)bx * by);
    ppg_spiral_block_ranks(bx, by, rank.data());
    std::vector<unsigned int> own(ctx->nPix);
    if (ctx->nPix) HIP_CHECK(hipMemcpy(own.data(), ctx->d_pixels.p, (size_t)ctx->nPix * 4, hipMemcpyDeviceToHost));
    std::vector<std::vector<unsigned int>> lists((size_t)regions);
    for (unsigned int p : own) {
        const int x = (int)(p % (unsigned int)ctx->W), y = (int)(p / (unsigned int)ctx->W);
        const int r = (int)((long long)rank[(size_t)(y / bs) * bx + (x / bs)] * regions / (bx * by));
        lists[(size_t)r].push_back(p);
    }
    ctx->regionOffset.assign((size_t)regions + 1, 0u);
    std::vector<unsigned int> flat;
    flat.reserve(own.size());
    for (int r = 0; r < regions; ++r) { ctx->regionOffset[(size_t)r] = (unsigned int)flat.size(); flat.insert(flat.end(), lists[(size_t)r].begin(), lists[(size_t)r].end()); }
    ctx->regionOffset[(size_t)regions] = (unsigned int)flat.size();
    HIP_CHECK(ctx->d_regionPixels.reserve(std::max<size_t>(1, flat.size())));
    if (!flat.empty()) HIP_CHECK(hipMemcpyAsync(ctx->d_regionPixels.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (`flat` is pageable host memory)
    ctx->regionsBuilt = regions;
    return PPG_OK;
}

int renderPassesBody(ppg_ctx *ctx, int numPasses) {  // GP:1217-1286
    size_t n = (size_t)ctx->W * ctx->H;
    HIP_CHECK(hipMemsetAsync(ctx->d_image.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_sq.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_imageW.p, 0, n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_stats.p, 0, sizeof(BlockStats) * (size_t)ctx->nBlocks, ctx->stream));
    HIP_CHECK(ctx->d_tailLongest.reserve(PPG_TAIL_LOG + 1));
    HIP_CHECK(hipMemsetAsync(ctx->d_tailLongest.p, 0, (PPG_TAIL_LOG + 1) * 4, ctx->stream));
    ctx->tailLaunches = 0;
    ctx->passStart = std::chrono::steady_clock::now();
    ctx->passesLocal = 0;
    // rounds of the sampling-fraction optimiser (include/ppg.h): fractions frozen during a round, its records applied afterwards
    const bool rounds = ctx->loss != LOSS_NONE && ctx->isBuilt && !ctx->isFinalIter;
    const int roundPasses = rounds ? (int)ppg_adam_round_passes(ctx->sppPerPass, ctx->W, ctx->H, numPasses) : (ctx->isFinalIter ? ctx->maxBatchFinal : ctx->maxBatch);
    ctx->samplesLocal = 0;
    ctx->partialsPending = false; ctx->partialsExported = false;
    if (ctx->filtered) { int rc = prepareFootprint(ctx); if (rc) return rc; }
    if (ctx->isFinalIter && ctx->budgetType == 0 && numPasses > 0) return renderFinalGroups(ctx, numPasses);
    // Cancelled while a round hook is installed (a sharded render with a learned sampling fraction): the other ranks enter the hook of
    // EVERY remaining round of this call, so this rank keeps entering it too — with empty rounds (no paths, no records; the host marks its
    // status word) — instead of leaving for an exchange the others are not in.  They all see the status and abort together.
    // rounds by image region (include/ppg.h ppg_set_adam_regions): in a call of at most PPG_ADAM_REGION_MAX_PASSES passes a round is one pass
    // over one group of blocks
    int regions = 0;
    if (rounds && ctx->adamRegions > 1 && numPasses <= PPG_ADAM_REGION_MAX_PASSES) {
        regions = std::min(ctx->adamRegions, ((ctx->W + 31) / 32) * ((ctx->H + 31) / 32));
        int rc = buildRegionLists(ctx, regions);
        if (rc) return rc;
    }
    bool drain = false;
    for (int i = 0; i < numPasses;) {
        if (ctx->seesCancel()) {
            if (rounds && ctx->passHook) drain = true;
            else {
                // (a sharded time budget: the other ranks are about to ask the stop hook after the batch they are rendering — this rank asks it
                // too, once, so that they meet in the same exchange; the host's hook carries its status word there and every rank stops)
                if (ctx->budgetType == 1 && ctx->stopHook) (void)ctx->stopHook(ctx->stopHookUser, PPG_STOP_CANCELLED);
                break;
            }
        }
        const int batch = regions ? 1 : std::min(roundPasses, numPasses - i);
        int rc = PPG_OK;
        if (regions) {
            for (int r = 0; r < regions && !rc; ++r) {
                const unsigned int first = ctx->regionOffset[(size_t)r], count = ctx->regionOffset[(size_t)r + 1] - first;
                // (a group without pixels of this rank — or a cancelled rank kept in step — is an empty round: the hook calls match across ranks)
                rc = renderBatch(ctx, drain ? 0 : 1, true, nullptr, i + 1 >= numPasses && r + 1 == regions, ctx->d_regionPixels.p + first, drain ? 0u : count);
            }
        } else rc = renderBatch(ctx, drain ? 0 : batch, rounds, nullptr, i + batch >= numPasses);
        if (rc) return rc;
        ctx->passesRendered += batch; ctx->passesRenderedThisIter += batch; ctx->passesLocal += batch;
        ctx->samplesLocal += (uint64_t)ctx->nPix * batch * ctx->sppPerPass;
        i += batch;
        if (ctx->budgetType == 1) {  // seconds: the reference checks after every finished pass (GP:1259-1262)
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            int stop = (int)elapsedSeconds(ctx->startTime) > ctx->budget ? 1 : 0;  // `progress = (int) elapsed; shouldAbort = progress > m_budget`
            if (ctx->stopHook) stop = ctx->stopHook(ctx->stopHookUser, stop);           // sharded: the decision of rank 0 for all
            if (stop) break;
        } else if ((i & 63) < batch) {
            HIP_CHECK(hipStreamSynchronize(ctx->stream));  // bound the launch queue; also lets ppg_cancel() take effect
        }
    }
    // what the last batch still owes ("Stragglers"); in a sharded render with rounds whose stragglers' records are deferred, the round of the
    // last stragglers' records is one more call of the round hook on EVERY rank (include/ppg.h "STRAGGLERS")
    {
        const bool deferRounds = rounds && ctx->maxDepth < 0 && recordPositionsKnown(ctx->spatialFilter, ctx->doNee, ctx->nee);
        int rc = flushStragglers(ctx, deferRounds && ctx->passHook != nullptr);
        if (rc) return rc;
    }
    // a filtered film: the call's footprint becomes its image / squared image / weights and is added to the iteration's film
    // (sharded by tiles: once the ranks have exchanged their footprints' borders, this rank's targets only — a cancelled rank says so there)
    if (ctx->exchangesFootprints()) { int rc = exchangeFootprint(ctx, ctx->d_image.p, ctx->d_sq.p, ctx->d_imageW.p, ctx->d_film.p, ctx->d_filmW.p); if (rc) return rc; }
    else if (ctx->filtered) launchFilmResolve(ctx, ctx->d_image.p, ctx->d_sq.p, ctx->d_imageW.p, ctx->d_film.p, ctx->d_filmW.p);
    return ctx->seesCancel() ? PPG_ERR_CANCELLED : PPG_OK;
}

// The footprint hook's calls of a call (include/ppg.h "Footprint hook") are counted by what every rank knows — final flag, budget type, pass
// count, world —, and no way out of the call may skip one the peers are making: a rank that left early (cancelled, a failed launch, a failed
// round hook) still makes its NEXT due call, with zeros and its status, where all ranks then learn of it and make no further ones.
int renderPassesNoStat(ppg_ctx *ctx, int numPasses) {
    ctx->footDue = 0; ctx->footDone = 0; ctx->footFailed = false;
    if (ctx->exchangesFootprints()) {
        if (!ctx->footHook) { ctx->error = kShardedFilter; return PPG_ERR_STATE; }
        if (ctx->isFinalIter && ctx->budgetType == 0 && numPasses > 0) {
            const unsigned int G = (unsigned int)ppg_final_group_passes(numPasses), nGroups = ((unsigned int)numPasses + G - 1) / G;
            ctx->footDue = finalGroupsByRank(nGroups, (unsigned int)ctx->shardWorld) ? 0u : nGroups;
        } else ctx->footDue = 1;
    }
    int rc = renderPassesBody(ctx, numPasses);
    if (ctx->footDone < ctx->footDue && !ctx->footFailed) {
        const std::string why = ctx->error;
        const uint64_t floats = ppg_footprint_halo_floats(ctx->W, ctx->H, ctx->tileSize, ctx->shardWorld, ctx->rfBorder);
        void *buf = nullptr;  // (a rank that could not even allocate the buffer joins without one: the hook gives zeros of its own)
        if (ctx->d_halo.reserve(std::max<size_t>(1, (size_t)floats)) == hipSuccess && hipMemsetAsync(ctx->d_halo.p, 0, std::max<size_t>(1, (size_t)floats) * 4, ctx->stream) == hipSuccess &&
            hipStreamSynchronize(ctx->stream) == hipSuccess) buf = ctx->d_halo.p;
        else (void)hipGetLastError();
        ++ctx->footDone;
        (void)ctx->footHook(ctx->footHookUser, buf, floats, 1);
        ctx->footFailed = true;
        ctx->error = why.empty() ? "footprint hook failed" : why;
        if (rc == PPG_OK) rc = PPG_ERR_INVALID;
    }
    return rc;
}

int finishPasses(ppg_ctx *ctx, ppg_pass_stats *st) {  // GP:1288-1328
    if (ctx->partialsPending) { ctx->error = "the groups of this final iteration were not exchanged: ppg_final_partials / ppg_final_partials_commit before ppg_finish_passes"; return PPG_ERR_STATE; }
    const int n = ctx->W * ctx->H;
    const int N = ctx->passesLocal * ctx->sppPerPass;
    if (ctx->sampleCombination == 2) {  // inversevar: m_images.push_back(image->clone())
        ctx->images.emplace_back();
        HIP_CHECK(ctx->images.back().reserve(3 * (size_t)n));
        hipLaunchKernelGGL(k_normalise, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, ctx->d_image.p, ctx->d_imageW.p, ctx->images.back().p);
    }
    hipLaunchKernelGGL(k_variance, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, ctx->W, N, ctx->d_image.p, ctx->d_sq.p, ctx->d_imageW.p, ctx->d_var.p, ctx->d_lum.p);
    float *lum = ctx->h_lum;  // pinned
    if (ctx->h_statsCap < (size_t)ctx->nBlocks) {
        if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
        ctx->h_stats = nullptr; ctx->h_statsCap = 0;
        HIP_CHECK(hipHostMalloc((void **)&ctx->h_stats, (size_t)ctx->nBlocks * sizeof(BlockStats), hipHostMallocDefault));
        ctx->h_statsCap = (size_t)ctx->nBlocks;
    }
    BlockStats *bs = ctx->h_stats;
    HIP_CHECK(hipMemcpyAsync(lum, ctx->d_lum.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(bs, ctx->d_stats.p, (size_t)ctx->nBlocks * sizeof(BlockStats), hipMemcpyDeviceToHost, ctx->stream));
    unsigned int tailLongest[PPG_TAIL_LOG];
    const unsigned int nTails = std::min<unsigned int>(ctx->tailLaunches, PPG_TAIL_LOG);
    if (nTails) HIP_CHECK(hipMemcpyAsync(tailLongest, ctx->d_tailLongest.p, nTails * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    BlockStats c{};
    for (int k = 0; k < ctx->nBlocks; ++k) { const BlockStats &x = bs[k]; c.rays += x.rays; c.path_len += x.path_len; c.committed += x.committed; c.bvh_nodes += x.bvh_nodes; c.bvh_tris += x.bvh_tris; c.max_len = std::max(c.max_len, x.max_len); c.shade_common += x.shade_common; }
    if (ctx->debugBatch) fprintf(stderr, "[ppg passes] iter %d passes %d rays %llu path_len_sum %llu longest path finished by k_tail %llu\n", ctx->iter, ctx->passesLocal, (unsigned long long)c.rays, (unsigned long long)c.path_len, (unsigned long long)c.max_len);
    ctx->bvhNodesVisited += c.bvh_nodes; ctx->bvhTrisTested += c.bvh_tris; ctx->shadeCommonRays += c.shade_common;
    for (unsigned int k = 0; k < nTails; ++k) ctx->tailLongestSum += tailLongest[k];
    float variance = 0;  // summed in the reference's x-major order (GP:1303-1311)
    for (int k = 0; k < n; ++k) variance += lum[k];  // k = x * H + y
    variance /= (float)ctx->W * ctx->H * (N - 1);
    if (ctx->sampleCombination == 2) ctx->variances.push_back(variance);
    ctx->lastVariance = variance;
    ppg_pass_stats s{};
    s.seconds = elapsedSeconds(ctx->passStart);
    s.passes_rendered_total = ctx->passesRendered; s.passes_rendered_local = ctx->passesLocal; s.variance = variance;
    s.samples = ctx->samplesLocal;
    s.rays = c.rays; s.path_length_sum = c.path_len; s.vertices_committed = c.committed;
    ctx->lastStats = s;
    if (st) *st = s;
    ctx->timer.resolve();
    return PPG_OK;
}

int allocFilm(ppg_ctx *ctx) {
    size_t n = (size_t)ctx->W * ctx->H;
    HIP_CHECK(ctx->d_image.reserve(3 * n)); HIP_CHECK(ctx->d_sq.reserve(3 * n)); HIP_CHECK(ctx->d_imageW.reserve(n));
    HIP_CHECK(ctx->d_film.reserve(3 * n)); HIP_CHECK(ctx->d_filmW.reserve(n)); HIP_CHECK(ctx->d_var.reserve(3 * n));
    HIP_CHECK(ctx->d_lum.reserve(n)); HIP_CHECK(ctx->d_tmp.reserve(3 * n));
    if (ctx->h_lumCap < n) {
        if (ctx->h_lum) (void)hipHostFree(ctx->h_lum);
        ctx->h_lum = nullptr; ctx->h_lumCap = 0;
        HIP_CHECK(hipHostMalloc((void **)&ctx->h_lum, n * sizeof(float), hipHostMallocDefault));
        ctx->h_lumCap = n;
    }
    return PPG_OK;
}

int beginRender(ppg_ctx *ctx) {  // GP:1519-1550
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    if (!ctx->pathsReady) {  // buffers are sized by scene + shard; normally done by ppg_set_scene / ppg_set_shard
        int rc = allocPaths(ctx);
        if (rc) return rc;
        if ((rc = allocFilm(ctx))) return rc;
        ctx->pathsReady = true;
    }
    // new STree(scene->getAABB()), cubified (GP:850-860)
    float maxSize = 0;
    for (int a = 0; a < 3; ++a) maxSize = ppg_max(maxSize, ctx->aabbMax[a] - ctx->aabbMin[a]);
    {
        float sx = ctx->aabbMax[0] - ctx->aabbMin[0], sy = ctx->aabbMax[1] - ctx->aabbMin[1], sz = ctx->aabbMax[2] - ctx->aabbMin[2];
        maxSize = ppg_max(ppg_max(sx, sy), sz);
    }
    for (int a = 0; a < 3; ++a) {
        ctx->treeMin[a] = ctx->aabbMin[a];
        ctx->treeMax[a] = ctx->aabbMin[a] + maxSize;
        ctx->treeExt[a] = ctx->treeMax[a] - ctx->treeMin[a];  // AABB::getExtents() = max - min
    }
    ctx->snodes.assign(1, HostSNode());
    ctx->hdr.assign(1, LeafHdr{});
    // the initial sampling D-tree: one node, all sums 0 (DTree(), GP:376-381)
    HIP_CHECK(ctx->d_snodes[0].reserve(1));
    HIP_CHECK(hipMemsetAsync(ctx->d_snodes[0].p, 0, sizeof(SNode), ctx->stream));
    ctx->cur = 0;
    ctx->hdr[0].s_base = 0; ctx->hdr[0].s_num = 1;
    {   // the root node goes to the device once; from here on the device owns the S-tree (refineDevice) and the host mirrors it
        int rc = uploadTree(ctx, true);
        if (rc) return rc;
        const unsigned int root = 0;
        HIP_CHECK(ctx->d_dfs[0].reserve(1));
        HIP_CHECK(hipMemcpy(ctx->d_dfs[0].p, &root, 4, hipMemcpyHostToDevice));
        ctx->dfsCur = 0; ctx->dfsCount = 1;
    }
    ctx->nSamplingNodes = 1; ctx->nBuildingNodes = 0;
    ctx->iter = 0; ctx->isFinalIter = false; ctx->isBuilt = false; ctx->iterOpen = false;
    size_t n = (size_t)ctx->W * ctx->H;
    HIP_CHECK(hipMemsetAsync(ctx->d_film.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_filmW.p, 0, n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_var.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_image.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_sq.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_imageW.p, 0, n * 4, ctx->stream));
    ctx->images.clear(); ctx->variances.clear();
#ifdef PPG_PROBE
    HIP_CHECK(ctx->d_probe.reserve(PPG_PROBE_SLOTS));
    HIP_CHECK(hipMemsetAsync(ctx->d_probe.p, 0, PPG_PROBE_SLOTS * 8, ctx->stream));
#endif
    ctx->startTime = std::chrono::steady_clock::now();
    ctx->passesRendered = 0; ctx->passesRenderedThisIter = 0;
    ctx->treeAlive = true;
    ctx->renderOpen = true;
    // ppg_cancel() is sticky: a cancel no render has acted on yet — it arrived while the scene was being set up, say, seconds of BVH build —
    // cancels THIS render; the flag is consumed here (it used to be cleared, and that cancel was lost).  One the previous render DID act on
    // (it returned PPG_ERR_CANCELLED, or left through a failing hook) is spent.
    {
        const bool pending = ctx->cancelled.exchange(false), spent = ctx->cancelSeen;
        ctx->cancelSeen = false;
        if (pending && !spent) { ctx->error = "cancelled before the render began"; return PPG_ERR_CANCELLED; }
    }
    return PPG_OK;
}

int beginIteration(ppg_ctx *ctx, bool isFinal) {  // GP:1378-1381
    ctx->isFinalIter = isFinal;
    ctx->iterOpen = false;
    size_t n = (size_t)ctx->W * ctx->H;
    HIP_CHECK(hipMemsetAsync(ctx->d_film.p, 0, 3 * n * 4, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_filmW.p, 0, n * 4, ctx->stream));
    const int rc = resetSDTree(ctx);
    ctx->iterOpen = rc == PPG_OK && !isFinal;
    return rc;
}

int dumpSDTreeFile(ppg_ctx *ctx, const char *path);

int endIteration(ppg_ctx *ctx) {  // GP:1417-1422
    if (ctx->dumpSDTree && !ctx->isFinalIter && !ctx->dumpPrefix.empty()) {
        char buf[1024];
        snprintf(buf, sizeof buf, "%s-%02d.sdt", ctx->dumpPrefix.c_str(), ctx->iter);
        int rc = dumpSDTreeFile(ctx, buf);
        if (rc) return rc;
    }
    ++ctx->iter;
    ctx->passesRenderedThisIter = 0;
    return PPG_OK;
}

int endRender(ppg_ctx *ctx) {  // GP:1567-1582
    ctx->joinTree();
    ctx->renderOpen = false;
#ifdef PPG_PROBE
    if (ctx->d_probe.p) {
        unsigned long long h[PPG_PROBE_SLOTS];
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        HIP_CHECK(hipMemcpy(h, ctx->d_probe.p, sizeof h, hipMemcpyDeviceToHost));
        fprintf(stderr, "[ppg probe] lone_bounces %llu coop_rays %llu coop_steps %llu cycles:", h[20], h[22], h[21]);
        for (int k = 0; k <= 11; ++k) fprintf(stderr, " s%d=%llu", k, h[k]);
        fprintf(stderr, "\n");
    }
#endif
    if (ctx->sampleCombination == 2 && !ctx->images.empty()) {
        const int n = ctx->W * ctx->H;
        HIP_CHECK(hipMemsetAsync(ctx->d_film.p, 0, 3 * (size_t)n * 4, ctx->stream));
        std::vector<float> ones((size_t)n, 1.0f);
        HIP_CHECK(hipMemcpyAsync(ctx->d_filmW.p, ones.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        size_t begin = ctx->images.size() - std::min(ctx->images.size(), (size_t)4);
        float totalWeight = 0;
        for (size_t i = begin; i < ctx->variances.size(); ++i) totalWeight += 1.0f / ctx->variances[i];
        for (size_t i = begin; i < ctx->images.size(); ++i) {
            float mult = 1.0f / ctx->variances[i] / totalWeight;
            hipLaunchKernelGGL(k_axpy, dim3((3 * n + 255) / 256), dim3(256), 0, ctx->stream, 3 * n, mult, ctx->images[i].p, ctx->d_film.p);
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PPG_OK;
}

bool doNeeWithSpp(const ppg_ctx *ctx, int spp) {  // GP:1331-1340
    switch (ctx->nee) {
        case NEE_NEVER: return false;
        case NEE_KICKSTART: return spp < 128;
        default: return true;
    }
}

int renderSPP(ppg_ctx *ctx) {  // GP:1342-1426
    size_t sampleCount = (size_t)ctx->budget;
    int nPasses = (int)std::ceil(sampleCount / (float)ctx->sppPerPass);
    float currentVarAtEnd = std::numeric_limits<float>::infinity();
    while (ctx->passesRendered < nPasses) {
        const int sppRendered = ctx->passesRendered * ctx->sppPerPass;
        ctx->doNee = doNeeWithSpp(ctx, sppRendered);
        int remainingPasses = nPasses - ctx->passesRendered;
        int passesThisIteration = std::min(remainingPasses, 1 << ctx->iter);
        if (remainingPasses - passesThisIteration < 2 * passesThisIteration) passesThisIteration = remainingPasses;
        int rc = beginIteration(ctx, passesThisIteration >= remainingPasses);
        if (rc) return rc;
        ppg_pass_stats st;
        if ((rc = renderPassesNoStat(ctx, passesThisIteration))) return rc;
        if ((rc = finishPasses(ctx, &st))) return rc;
        float variance = st.variance;
        const float lastVarAtEnd = currentVarAtEnd;
        currentVarAtEnd = passesThisIteration * variance / remainingPasses;
        remainingPasses -= passesThisIteration;
        if (ctx->sampleCombination == 1 && remainingPasses > 0 &&
            (remainingPasses < passesThisIteration || (sppRendered > 256 && currentVarAtEnd > lastVarAtEnd))) {
            ctx->isFinalIter = true;
            if ((rc = renderPassesNoStat(ctx, remainingPasses))) return rc;
            if ((rc = finishPasses(ctx, &st))) return rc;
        }
        if ((rc = buildSDTree(ctx, nullptr))) return rc;
        if ((rc = endIteration(ctx))) return rc;
    }
    return PPG_OK;
}

int renderTime(ppg_ctx *ctx) {  // GP:1434-1514
    float nSeconds = ctx->budget;
    float currentVarAtEnd = std::numeric_limits<float>::infinity();
    float elapsed = 0;
    while (elapsed < nSeconds) {
        const int sppRendered = ctx->passesRendered * ctx->sppPerPass;
        ctx->doNee = doNeeWithSpp(ctx, sppRendered);
        float remainingTime = nSeconds - elapsed;
        const int passesThisIteration = 1 << ctx->iter;
        const auto startIter = std::chrono::steady_clock::now();
        int rc = beginIteration(ctx, false);
        if (rc) return rc;
        ppg_pass_stats st;
        if ((rc = renderPassesNoStat(ctx, passesThisIteration))) return rc;
        if ((rc = finishPasses(ctx, &st))) return rc;
        float variance = st.variance;
        const float secondsIter = elapsedSeconds(startIter);
        const float lastVarAtEnd = currentVarAtEnd;
        currentVarAtEnd = secondsIter * variance / remainingTime;
        remainingTime -= secondsIter;
        if (ctx->sampleCombination == 1 && remainingTime > 0 &&
            (remainingTime < secondsIter || (sppRendered > 256 && currentVarAtEnd > lastVarAtEnd))) {
            ctx->isFinalIter = true;
            do {
                if ((rc = renderPassesNoStat(ctx, passesThisIteration))) return rc;
                if ((rc = finishPasses(ctx, &st))) return rc;
                elapsed = elapsedSeconds(ctx->startTime);
            } while (elapsed < nSeconds);
        }
        if ((rc = buildSDTree(ctx, nullptr))) return rc;
        if ((rc = endIteration(ctx))) return rc;
        elapsed = elapsedSeconds(ctx->startTime);
    }
    return PPG_OK;
}

// gather one kind of D-trees per S-tree leaf into host arrays (expands shared sampling blocks)
int gatherDTrees(ppg_ctx *ctx, int which, std::vector<float> &sums, std::vector<uint16_t> &children, std::vector<uint64_t> *fixed) {
    sums.clear(); children.clear(); if (fixed) fixed->clear();
    if (which == 0) {
        std::vector<SNode> pool(ctx->nSamplingNodes);
        if (!pool.empty()) HIP_CHECK(hipMemcpy(pool.data(), ctx->d_snodes[ctx->cur].p, pool.size() * sizeof(SNode), hipMemcpyDeviceToHost));
        for (unsigned int leaf : ctx->leaves) {
            const LeafHdr &h = ctx->hdr[leaf];
            for (unsigned int n = 0; n < h.s_num; ++n)
                for (int j = 0; j < 4; ++j) {
                    sums.push_back(pool[h.s_base + n].sum[j]); children.push_back(pool[h.s_base + n].child[j]);
                    if (fixed) fixed->push_back(0);
                }
        }
    } else {
        std::vector<ushort4> ch(ctx->nBuildingNodes);
        std::vector<unsigned long long> acc(ctx->nBuildingNodes * 4);
        if (!ch.empty()) {
            HIP_CHECK(hipMemcpy(ch.data(), ctx->d_bchild.p, ch.size() * sizeof(ushort4), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(acc.data(), ctx->d_bacc.p, acc.size() * 8, hipMemcpyDeviceToHost));
        }
        std::vector<LeafHdr> dh(ctx->hdr.size());
        HIP_CHECK(hipMemcpy(dh.data(), ctx->d_hdr.p, dh.size() * sizeof(LeafHdr), hipMemcpyDeviceToHost));
        for (unsigned int leaf : ctx->leaves) {
            const LeafHdr &h = dh[leaf];
            for (unsigned int n = 0; n < h.b_num; ++n) {
                const unsigned short cc[4] = {ch[h.b_base + n].x, ch[h.b_base + n].y, ch[h.b_base + n].z, ch[h.b_base + n].w};
                for (int j = 0; j < 4; ++j) {
                    uint64_t a = acc[(size_t)(h.b_base + n) * 4 + j];
                    sums.push_back(cc[j] == 0 ? ppg_from_fixed(a) : 0.0f); children.push_back(cc[j]);
                    if (fixed) fixed->push_back(a);
                }
            }
        }
    }
    return PPG_OK;
}

int dumpSDTreeFile(ppg_ctx *ctx, const char *path) {  // GP:1191-1208 + STree::dump GP:945-951 + DTreeWrapper::dump GP:699-711
    std::vector<SNode> pool(ctx->nSamplingNodes);
    if (!pool.empty()) HIP_CHECK(hipMemcpy(pool.data(), ctx->d_snodes[ctx->cur].p, pool.size() * sizeof(SNode), hipMemcpyDeviceToHost));
    FILE *f = fopen(path, "wb");
    if (!f) { ctx->error = std::string("cannot open ") + path; return PPG_ERR_INVALID; }
    fwrite(ctx->scene.cam.c2w, 4, 16, f);
    // STreeNode::forEachLeaf (GP:796-813): depth-first, child 0 before child 1
    struct E { size_t idx; float p[3], s[3]; };
    std::vector<E> st;
    E root; root.idx = 0;
    for (int a = 0; a < 3; ++a) { root.p[a] = ctx->treeMin[a]; root.s[a] = ctx->treeMax[a] - ctx->treeMin[a]; }
    st.push_back(root);
    while (!st.empty()) {
        E e = st.back(); st.pop_back();
        const HostSNode &n = ctx->snodes[e.idx];
        if (n.isLeaf()) {
            const LeafHdr &h = ctx->hdr[e.idx];
            if (h.s_statw > 0) {
                float mean = 0;
                if (h.s_statw != 0) { const float factor = 1 / (PPG_PI_F * 4 * h.s_statw); mean = factor * h.s_sum; }
                float hd[7] = {e.p[0], e.p[1], e.p[2], e.s[0], e.s[1], e.s[2], mean};
                fwrite(hd, 4, 7, f);
                uint64_t sw = (uint64_t)h.s_statw, nn = h.s_num;
                fwrite(&sw, 8, 1, f); fwrite(&nn, 8, 1, f);
                for (unsigned int k = 0; k < h.s_num; ++k)
                    for (int j = 0; j < 4; ++j) { fwrite(&pool[h.s_base + k].sum[j], 4, 1, f); fwrite(&pool[h.s_base + k].child[j], 2, 1, f); }
            }
        } else {
            E c0 = e, c1 = e;
            c0.s[n.axis] /= 2; c1.s[n.axis] = c0.s[n.axis];
            c0.idx = n.child[0]; c1.idx = n.child[1];
            c1.p[n.axis] += c1.s[n.axis];
            st.push_back(c1); st.push_back(c0);
        }
    }
    fclose(f);
    return PPG_OK;
}

// ppg_load_sdtree (include/ppg.h "Loading a dumped SD-tree"): the file through ppg_sdt_load.h — every refusal is decided there, on the host,
// before the context is touched —, then the state that buildSDTree + endIteration of iteration opts.iter - 1 leave.
int loadSDTreeFile(ppg_ctx *ctx, const char *path, int iter, int passesRendered) {
    std::vector<uint8_t> bytes;
    {
        FILE *f = fopen(path, "rb");
        if (!f) { ctx->error = std::string("ppg_load_sdtree: cannot open ") + path; return PPG_ERR_INVALID; }
        uint8_t buf[1 << 16];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) { ctx->error = std::string("ppg_load_sdtree: cannot read ") + path; return PPG_ERR_INVALID; }
    }
    ppg_sdt::Tree T;
    {
        std::string why;
        const int rc = ppg_sdt::importTree(bytes.data(), bytes.size(), ctx->treeMin, ctx->treeMax, ctx->spatialFilter, ppg_sdt::Limits(), T, why);
        if (rc) { ctx->error = std::string("ppg_load_sdtree: ") + path + ": " + why; return rc; }
    }
    bytes.clear(); bytes.shrink_to_fit();
    const size_t nS = T.axis.size(), nD = T.nodes.size();
    std::vector<SNode> pool(nD);
    std::vector<ushort4> bchild(nD);
    for (size_t k = 0; k < nD; ++k) {
        const ppg_sdt::Node &n = T.nodes[k];
        for (int j = 0; j < 4; ++j) { pool[k].sum[j] = n.sum[j]; pool[k].child[j] = n.child[j]; }
        pool[k].pad[0] = pool[k].pad[1] = 0;
        bchild[k] = make_ushort4(n.child[0], n.child[1], n.child[2], n.child[3]);
    }
    ctx->joinTree();
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // the sampling pool; the building trees have its topology and empty accumulators until the next ppg_begin_iteration resets them
    HIP_CHECK(ctx->d_snodes[ctx->cur].reserve(nD));
    HIP_CHECK(ctx->d_bchild.reserve(nD));
    HIP_CHECK(ctx->d_bacc.reserve(nD * 4));
    HIP_CHECK(ctx->d_dfs[0].reserve(T.dfsRightFirst.size()));
    HIP_CHECK(hipMemcpyAsync(ctx->d_snodes[ctx->cur].p, pool.data(), nD * sizeof(SNode), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(ctx->d_bchild.p, bchild.data(), nD * sizeof(ushort4), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_bacc.p, 0, nD * 4 * 8, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(ctx->d_dfs[0].p, T.dfsRightFirst.data(), T.dfsRightFirst.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ctx->dfsCur = 0; ctx->dfsCount = (unsigned int)T.dfsRightFirst.size();
    ctx->snodes.assign(nS, HostSNode());
    ctx->hdr.assign(nS, LeafHdr{});  // theta and the optimiser's state: a fresh leaf's (the file does not carry them)
    for (size_t i = 0; i < nS; ++i) {
        ctx->snodes[i].axis = T.axis[i]; ctx->snodes[i].child[0] = T.children[2 * i]; ctx->snodes[i].child[1] = T.children[2 * i + 1];
        if (!ctx->snodes[i].isLeaf()) continue;
        const ppg_sdt::Leaf &l = T.hdr[i];
        LeafHdr &h = ctx->hdr[i];
        h.s_base = l.base; h.s_num = l.num; h.s_sum = l.sum; h.s_statw = l.statw; h.s_depth = l.depth;
        h.b_base = l.base; h.b_num = l.num; h.b_depth = l.depth;
        h.b_statw = l.statw;  // as k_dtree_build leaves it: the next refine splits by it
    }
    ctx->nSamplingNodes = nD; ctx->nBuildingNodes = nD;
    { int rc = uploadTree(ctx, true); if (rc) return rc; }  // S-tree, headers, leaf list, lookup grid; waits for the copies above
    ctx->isBuilt = true; ctx->isFinalIter = false; ctx->iterOpen = false;
    ctx->iter = iter; ctx->passesRendered = passesRendered; ctx->passesRenderedThisIter = 0;
    return PPG_OK;
}

// Host tables to the device.  One call per table: into `buf`, grown to at least minCap elements; it gives the device pointer, or null for
// an empty table that asked for no capacity (the optional ones).  After a failure the later calls do nothing: `e` keeps the first error.
struct Upload {
    hipError_t e = hipSuccess;
    template <typename T> const T *operator()(DevBuf<T> &buf, const std::vector<T> &v, size_t minCap = 0) {
        if (e == hipSuccess) e = buf.reserve(std::max(v.size(), minCap));
        if (e == hipSuccess && !v.empty()) e = hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e == hipSuccess && (!v.empty() || minCap) ? buf.p : nullptr;
    }
};

// Every table of H into the context's buffers; S: H's scalars with the pointers of the uploaded tables.
int uploadScene(ppg_ctx *ctx, const HostScene &H, DevScene &S) {
    Upload up;
    S = H.scene;
    S.tris = up(ctx->d_tris, H.tris, 3); S.accel = up(ctx->d_accel, H.accel, 3); S.accel_small = up(ctx->d_accelSmall, H.accelSmall, 3);
    S.normals = up(ctx->d_normals, H.normals); S.uvs = up(ctx->d_uvs, H.uvs);
    S.bvh = up(ctx->d_bvh, H.nodes, 1); S.bvh4 = up(ctx->d_bvh4, H.nodes4q); S.bvh_top = up(ctx->d_bvhTop, H.topCut, 2);
    S.materials = up(ctx->d_materials, H.mats); S.emitters = up(ctx->d_emitters, H.ems); S.rtrans = up(ctx->d_rtrans, H.rtrans);
    S.mfd = up(ctx->d_mfd, H.mfd); S.coat = up(ctx->d_coat, H.coat); S.blend = up(ctx->d_blend, H.blend);
    std::vector<DevTex> textures = H.textures;  // ... completed by the texel pointers
    ctx->d_texTexels.clear();
    ctx->d_texTexels.resize(textures.size());
    for (size_t i = 0; i < textures.size(); ++i) textures[i].texels = up(ctx->d_texTexels[i], H.texTexels[i]);
    S.textures = up(ctx->d_textures, textures);
    S.em_texels = up(ctx->d_emTexels, H.envTexels); S.em_cdf_rows = up(ctx->d_emCdfRows, H.envCdfRows);
    S.em_cdf_cols = up(ctx->d_emCdfCols, H.envCdfCols); S.em_row_weights = up(ctx->d_emRowWeights, H.envRowWeights);
    S.em_sel_cdf = up(ctx->d_emSel, H.emSel); S.em_area_cdf = up(ctx->d_emArea, H.emArea); S.em_info = up(ctx->d_emInfo, H.emInfo);
    S.em_tris = up(ctx->d_emTris, H.emTris); S.em_normals = up(ctx->d_emNrm, H.emNormals);
    S.delta = up(ctx->d_delta, H.delta); S.shapes = up(ctx->d_shapes, H.shapes); S.spheres = up(ctx->d_spheres, H.spheres);
    MediaArgs &M = ctx->mediaArgs;
    M = MediaArgs{};
    M.media = up(ctx->d_media, H.media); M.prim_media = up(ctx->d_primMedia, H.primMedia);
    M.camera_medium = H.cameraMedium; M.n_media = (int)(H.media.size() / PPG_MEDIUM_STRIDE);
    HetArgs &V = ctx->hetArgs;
    V = HetArgs{};
    V.volumes = up(ctx->d_volumes, H.volumes); V.pool = up(ctx->d_volPool, H.volPool); V.het = up(ctx->d_het, H.het);
    V.n_volumes = (int)(H.volumes.size() / PPG_VOLUME_STRIDE);
    ctx->hetMedium.assign(H.het.size() / PPG_HET_STRIDE, 0);
    for (size_t k = 0; k < ctx->hetMedium.size(); ++k) ctx->hetMedium[k] = __builtin_bit_cast(int, H.het[PPG_HET_STRIDE * k].x) != 0;
    HIP_CHECK(up.e);
    if (!H.media.empty() && (!M.media || !M.prim_media)) { ctx->error = "internal: device scene incomplete"; return PPG_ERR_STATE; }
    if (!H.het.empty() && (!V.volumes || !V.pool || !V.het || !M.media)) { ctx->error = "internal: device scene incomplete"; return PPG_ERR_STATE; }
    // Every array the path kernels walk must be there before a launch can chase it: an unset pointer here is a hung GPU, not a wrong pixel
    // (round 5 lost 40 GPU minutes to five assignments that an edit had turned into a comment).
    if (!S.materials || !S.bvh4 || (S.n_tris > 0 && (!S.tris || !S.accel || !S.bvh)) || (S.n_spheres > 0 && !S.spheres) || (S.n_delta > 0 && !S.delta) ||
        (S.n_shapes > 0 && !S.shapes) || !S.em_sel_cdf || !S.em_info || !S.em_area_cdf || !S.em_tris || (S.env.w == 2.0f && !S.em_texels)) {
        ctx->error = "internal: device scene incomplete";
        return PPG_ERR_STATE;
    }
    return PPG_OK;
}

// scene and shard size the per-pass buffers (path state, vertex slots, queues, film)
int sizeBuffers(ppg_ctx *ctx) {
    ctx->pathsReady = false;
    if (!ctx->haveScene) return PPG_OK;
    int rc = allocPaths(ctx);
    if (rc) return rc;
    if ((rc = allocFilm(ctx))) return rc;
    if ((rc = presizeRounds(ctx))) return rc;
    ctx->pathsReady = true;
    return PPG_OK;
}

// The per-material side lists: kept until replaced, validated against the scene and packed by ppg_set_scene.  A null list with n > 0
// clears the list, or is refused where the list has no "none" (nullClears = false).
template <typename T> int setSideList(ppg_ctx *ctx, const char *name, std::vector<T> &list, const T *items, uint32_t n, bool nullClears) {
    if (ctx->renderOpen) { ctx->error = std::string(name) + ": not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && !items && !nullClears) { ctx->error = std::string(name) + ": no list"; return PPG_ERR_INVALID; }
    if (!items) n = 0;
    list.assign(items, items + n);
    return PPG_OK;
}
}  // namespace

// ================================================================================================
// C-ABI (include/ppg.h)
// ================================================================================================
extern "C" {

void ppg_config_default(ppg_config *cfg) {
    memset(cfg, 0, sizeof *cfg);
    cfg->nee = "never"; cfg->sampleCombination = "automatic"; cfg->spatialFilter = "nearest"; cfg->directionalFilter = "nearest";
    cfg->bsdfSamplingFractionLoss = "none"; cfg->sdTreeMaxMemory = -1; cfg->sTreeThreshold = 12000; cfg->dTreeThreshold = 0.01f;
    cfg->bsdfSamplingFraction = 0.5f; cfg->sppPerPass = 4; cfg->budgetType = "seconds"; cfg->budget = 300.0f; cfg->dumpSDTree = 0;
    cfg->rrDepth = 5; cfg->maxDepth = -1; cfg->strictNormals = 0; cfg->hideEmitters = 0; cfg->seed = 0; cfg->device = 0; cfg->dumpPrefix = nullptr;
}

const char *ppg_description(void) { return "Guided path tracer"; }

int32_t ppg_adam_round_passes(int32_t spp_per_pass, int32_t width, int32_t height, int32_t n_passes) {
    const uint64_t perPass = (uint64_t)std::max(1, spp_per_pass) * (uint64_t)std::max(1, width) * (uint64_t)std::max(1, height);
    int32_t r = 1;
    while (r * 2 <= PPG_ADAM_ROUND_MAX_PASSES && r * 4 <= n_passes && (uint64_t)(r * 2) * perPass <= PPG_ADAM_ROUND_MAX_PATHS) r *= 2;
    return r;
}

int ppg_create(const ppg_config *cfg, ppg_ctx **out) {
    if (!cfg || !out) { g_createError = "null argument"; return PPG_ERR_INVALID; }
    std::unique_ptr<ppg_ctx> c(new ppg_ctx());
#define PARSE(field, dflt, target, ...)                                                                                  \
    c->target = parseEnum(cfg->field, dflt, {__VA_ARGS__});                                                              \
    if (c->target < 0) { g_createError = std::string("invalid value for '" #field "': ") + (cfg->field ? cfg->field : ""); return PPG_ERR_INVALID; }
    PARSE(nee, "never", nee, "never", "kickstart", "always")
    PARSE(sampleCombination, "automatic", sampleCombination, "discard", "automatic", "inversevar")
    PARSE(spatialFilter, "nearest", spatialFilter, "nearest", "stochastic", "box")
    PARSE(directionalFilter, "nearest", directionalFilter, "nearest", "box")
    PARSE(bsdfSamplingFractionLoss, "none", loss, "none", "kl", "var")
    PARSE(budgetType, "seconds", budgetType, "spp", "seconds")
#undef PARSE
    c->sdTreeMaxMemory = cfg->sdTreeMaxMemory; c->sTreeThreshold = cfg->sTreeThreshold; c->dTreeThreshold = cfg->dTreeThreshold;
    c->bsdfSamplingFraction = cfg->bsdfSamplingFraction; c->sppPerPass = cfg->sppPerPass; c->budget = cfg->budget;
    c->dumpSDTree = cfg->dumpSDTree != 0; c->rrDepth = cfg->rrDepth; c->maxDepth = cfg->maxDepth;
    c->strictNormals = cfg->strictNormals != 0; c->hideEmitters = cfg->hideEmitters != 0; c->seed = cfg->seed; c->device = cfg->device;
    if (cfg->dumpPrefix) c->dumpPrefix = cfg->dumpPrefix;
    {   // tuning switches (performance experiments only; results do not depend on them)
        if (const char *e = getenv("PPG_TAIL_THRESHOLD")) c->tailThreshold = (unsigned int)std::max(0ll, atoll(e));
        if (const char *e = getenv("PPG_TAIL_MIN")) c->tailMin = (unsigned int)std::max(1ll, atoll(e));
        if (const char *e = getenv("PPG_TAIL_DIV")) c->tailDiv = (unsigned int)std::max(1ll, atoll(e));
        if (const char *e = getenv("PPG_BATCH_PATHS")) c->tuneBatchPaths = (size_t)std::max(1ll, atoll(e));
        if (const char *e = getenv("PPG_BLOCKS")) c->tuneBlocks = std::max(1, atoi(e));
        c->tuneForceBvh = getenv("PPG_FORCE_BVH") != nullptr;
        c->tuneNoSort = getenv("PPG_NO_SORT") != nullptr;
        c->tuneNoSplit = getenv("PPG_NO_SPLIT") != nullptr;
        c->tuneNoSortFirst = getenv("PPG_NO_SORT_FIRST") != nullptr;
        c->tuneNoOverlap = getenv("PPG_NO_OVERLAP") != nullptr;
        c->tuneNoSortedCommit = getenv("PPG_NO_SORTED_COMMIT") != nullptr;
        c->tuneAdamUnordered = getenv("PPG_ADAM_UNORDERED") != nullptr;
        c->tuneNoAside = getenv("PPG_NO_ASIDE") != nullptr;
        if (const char *e = getenv("PPG_SPLAT_LDS_NODES")) c->tuneSplatLdsNodes = (unsigned int)std::max(0, std::min((int)PPG_SPLAT_NODES, atoi(e)));
        if (const char *e = getenv("PPG_BULK_BOUNCES")) c->tuneBulkBounces = std::max(0, atoi(e));
        if (const char *e = getenv("PPG_BOUNCE_MARGIN")) c->bounceMargin = std::max(0, atoi(e));
        c->debugBatch = getenv("PPG_DEBUG_BATCH") != nullptr;
        if (const char *e = getenv("PPG_TAIL_BLOCKS")) c->tuneTailBlocks = std::max(1, atoi(e));
        if (const char *e = getenv("PPG_FINAL_BATCH")) c->tuneFinalBatch = std::max(1, atoi(e));
        if (const char *e = getenv("PPG_PATH_LAYOUT")) c->tunePathLayout = !strcmp(e, "aos") ? 2 : (!strcmp(e, "soa") ? 1 : 0);
        if (const char *e = getenv("PPG_BLOCKS_SMALL")) c->tuneBlocksSmall = std::max(0, atoi(e));
        if (const char *e = getenv("PPG_SMALL_PATHS")) c->tuneSmallPaths = (size_t)std::max(0ll, atoll(e));
        if (const char *e = getenv("PPG_BVH_LEAF")) c->tuneBvhLeaf = std::max(1, std::min(8, atoi(e)));
        if (const char *e = getenv("PPG_BVH_PAD")) c->tuneBvhPad = (float)atof(e);
        if (const char *e = getenv("PPG_SPLIT_DEPTH")) c->tuneSplitDepth = std::max(0, atoi(e));
        c->tuneFinalHalves = getenv("PPG_FINAL_HALVES") != nullptr;
        c->tuneNoTopCut = getenv("PPG_NO_TOPCUT") != nullptr;
    }
    if (c->sppPerPass <= 0) { g_createError = "sppPerPass must be > 0"; return PPG_ERR_INVALID; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_createError = std::string("no HIP device available: ") + hipGetErrorString(e); return PPG_ERR_DEVICE; }
    if (c->device < 0 || c->device >= ndev) { g_createError = "device ordinal out of range"; return PPG_ERR_INVALID; }
    if ((e = hipSetDevice(c->device)) != hipSuccess || (e = hipStreamCreate(&c->stream)) != hipSuccess || (e = hipStreamCreate(&c->stream2)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming)) != hipSuccess ||
        (e = hipStreamCreate(&c->stream3)) != hipSuccess || (e = hipEventCreateWithFlags(&c->evTreeFork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipStreamCreate(&c->stream4)) != hipSuccess || (e = hipEventCreateWithFlags(&c->evStragFork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->evStragDone, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->evSplatDone, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&c->evAdamDone, hipEventDisableTiming)) != hipSuccess) {
        g_createError = std::string("HIP init failed: ") + hipGetErrorString(e);
        return PPG_ERR_DEVICE;
    }
    *out = c.release();
    return PPG_OK;
}

void ppg_destroy(ppg_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); }
    g_blockCache.settle();
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    if (ctx->stream4) (void)hipStreamSynchronize(ctx->stream4);
    g_blockCache.settle();
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->stream4) (void)hipStreamDestroy(ctx->stream4);
    for (hipEvent_t ev : {ctx->evStragFork, ctx->evStragDone}) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {ctx->evTreeFork, ctx->evSplatDone, ctx->evAdamDone}) if (ev) (void)hipEventDestroy(ev);
    if (ctx->evFork) (void)hipEventDestroy(ctx->evFork);
    if (ctx->evJoin) (void)hipEventDestroy(ctx->evJoin);
    ctx->timer.resolve();
    for (auto e : ctx->timer.pool) (void)hipEventDestroy(e);
    if (ctx->h_lum) (void)hipHostFree(ctx->h_lum);
    if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
    if (ctx->h_round) (void)hipHostFree(ctx->h_round);
    hipStream_t s = ctx->stream;
    delete ctx;
    if (s) (void)hipStreamDestroy(s);
}

const char *ppg_last_error(const ppg_ctx *ctx) { return ctx ? ctx->error.c_str() : g_createError.c_str(); }

int ppg_set_scene(ppg_ctx *ctx, const ppg_scene *s) {
    const SceneInputs in{s, ctx->materialTextures, ctx->microfacet, ctx->coatings, ctx->blends, ctx->deltaEmitters, ctx->shapes,
                         ctx->lensOn ? &ctx->lens : nullptr, ctx->tuneBvhPad, ctx->tuneBvhLeaf, ctx->tuneNoTopCut, ctx->mediaList.n_media ? &ctx->mediaList : nullptr,
                         ctx->volumesList.n_entries ? &ctx->volumesList : nullptr};
    if (!sceneComplete(in)) { ctx->error = "incomplete scene"; return PPG_ERR_INVALID; }
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    HostScene H;
    if (int rc = buildScene(in, H, ctx->error)) return rc;  // refused: nothing of the context has been touched, the previous scene stays set
    if (!H.media.empty() && ctx->shardWorld > 1) { ctx->error = kShardedMedia; return PPG_ERR_INVALID; }
    // From here on the buffers the previous scene points into are re-used: no scene is set until the new one is complete
    ctx->haveScene = false; ctx->treeAlive = false; ctx->renderOpen = false; ctx->pathsReady = false;
    DevScene S;
    if (int rc = uploadScene(ctx, H, S)) return rc;
    ctx->scene = S;
    for (int a = 0; a < 3; ++a) { ctx->geomMin[a] = H.geomMin[a]; ctx->geomMax[a] = H.geomMax[a]; ctx->aabbMin[a] = H.aabbMin[a]; ctx->aabbMax[a] = H.aabbMax[a]; }
    ctx->sceneDelta = std::move(H.deltaEmitters);
    ctx->fullMaterials = H.fullMaterials; ctx->nMaterials = H.nMaterials;
    ctx->ldsNodes = H.ldsNodes; ctx->ldsTris = H.ldsTris;
    ctx->W = H.W; ctx->H = H.H;
    ctx->haveScene = true;
    return sizeBuffers(ctx);
}

int ppg_set_shard(ppg_ctx *ctx, int32_t rank, int32_t world, int32_t tile_size) {
    (void)hipSetDevice(ctx->device);
    ctx->quiesce();
    if (world < 1 || rank < 0 || rank >= world || tile_size < 1) { ctx->error = "bad shard"; return PPG_ERR_INVALID; }
    if (world > 1 && ctx->filtered && !ctx->footHook) { ctx->error = kShardedFilter; return PPG_ERR_INVALID; }
    if (world > 1 && ctx->haveScene && ctx->mediaArgs.media) { ctx->error = kShardedMedia; return PPG_ERR_INVALID; }
    ctx->shardRank = rank; ctx->shardWorld = world; ctx->tileSize = tile_size;
    return sizeBuffers(ctx);
}

// every entry point re-selects the context's device: the caller (torch / RCCL in a multi-GPU process) may have changed it
// ... and names the context's stream as the one buffer growth is ordered on (StreamScope)
#define NEED_SCENE (void)hipSetDevice(ctx->device); StreamScope scope_(ctx->stream); if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
#define NEED_TREE (void)hipSetDevice(ctx->device); StreamScope scope_(ctx->stream); if (!ctx->treeAlive) { ctx->error = "render not begun"; return PPG_ERR_STATE; } ctx->joinTree();

int ppg_begin_render(ppg_ctx *ctx) { NEED_SCENE return beginRender(ctx); }
int ppg_begin_iteration(ppg_ctx *ctx, int32_t is_final) { NEED_TREE return beginIteration(ctx, is_final != 0); }
int ppg_set_final(ppg_ctx *ctx, int32_t is_final) { ctx->isFinalIter = is_final != 0; return PPG_OK; }
int ppg_set_do_nee(ppg_ctx *ctx, int32_t do_nee) { ctx->doNee = do_nee != 0; return PPG_OK; }
int ppg_render_passes_nostat(ppg_ctx *ctx, int32_t n) { NEED_TREE return renderPassesNoStat(ctx, n); }
int ppg_finish_passes(ppg_ctx *ctx, ppg_pass_stats *st) { NEED_TREE return finishPasses(ctx, st); }
int ppg_render_passes(ppg_ctx *ctx, int32_t n, ppg_pass_stats *st) {
    NEED_TREE
    int rc = renderPassesNoStat(ctx, n);
    if (rc && rc != PPG_ERR_CANCELLED) return rc;
    int rc2 = finishPasses(ctx, st);
    return rc ? rc : rc2;
}
int ppg_build_sdtree(ppg_ctx *ctx, ppg_tree_stats *st) { NEED_TREE return buildSDTree(ctx, st); }
int ppg_end_iteration(ppg_ctx *ctx) { NEED_TREE return endIteration(ctx); }
int ppg_end_render(ppg_ctx *ctx) { NEED_TREE return endRender(ctx); }
int ppg_cancel(ppg_ctx *ctx) { ctx->cancelled.store(true); return PPG_OK; }
int ppg_debug_build_bvh(const float *positions, const uint32_t *indices, uint32_t n_triangles, float pad_abs, int32_t max_leaf,
                        void *nodes_out, uint32_t nodes_cap, uint32_t *n_nodes, uint32_t *order_out) {
    if (!positions || !indices || !n_nodes || n_triangles == 0) return PPG_ERR_INVALID;
    BvhBuilder bb;
    bb.maxLeaf = std::max(1, std::min(8, (int)max_leaf));
    bb.run(positions, indices, n_triangles, pad_abs);
    *n_nodes = (uint32_t)bb.nodes4q.size();
    if (nodes_out) memcpy(nodes_out, bb.nodes4q.data(), std::min<size_t>(nodes_cap, bb.nodes4q.size()) * sizeof(Bvh4QNode));
    if (order_out) memcpy(order_out, bb.order.data(), (size_t)n_triangles * sizeof(uint32_t));
    return PPG_OK;
}
// child k's box of a quantised node as the kernels' float decode gives it (bvh4q_load, trace_closest4_wave)
static void decodeChildBox(const Bvh4QNode &q, int k, float lo[3], float hi[3]) {
    const float s[3] = {BvhBuilder::scaleOf(q.exps & 255u), BvhBuilder::scaleOf((q.exps >> 8) & 255u), BvhBuilder::scaleOf((q.exps >> 16) & 255u)};
    const float org[3] = {q.ox, q.oy, q.oz};
    const unsigned int ql[3] = {q.qlox, q.qloy, q.qloz}, qh[3] = {q.qhix, q.qhiy, q.qhiz};
    for (int a = 0; a < 3; ++a) {
        lo[a] = org[a] + (float)((ql[a] >> (8 * k)) & 255u) * s[a];
        hi[a] = org[a] + (float)((qh[a] >> (8 * k)) & 255u) * s[a];
    }
}
int ppg_debug_bvh_stats(const float *positions, const uint32_t *indices, uint32_t n_triangles, float pad_abs, int32_t max_leaf, ppg_bvh_stats *out) {
    if (!positions || !indices || !out || n_triangles == 0) return PPG_ERR_INVALID;
    BvhBuilder bb;
    bb.maxLeaf = std::max(1, std::min(8, (int)max_leaf));
    const auto t0 = std::chrono::steady_clock::now();
    bb.run(positions, indices, n_triangles, pad_abs);
    const auto t1 = std::chrono::steady_clock::now();
    memset(out, 0, sizeof(*out));
    out->build_seconds = std::chrono::duration<double>(t1 - t0).count();
    out->n_nodes = (uint32_t)bb.nodes4q.size();
    out->n_binary_nodes = (uint32_t)bb.nodes.size();
    out->stack_need = (uint32_t)BvhBuilder::stackNeedOf(bb.nodes4);
    auto areaOf = [](const float lo[3], const float hi[3]) {
        const double d[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};
        return d[0] < 0 || d[1] < 0 || d[2] < 0 ? 0.0 : 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    };
    double rootArea = 0;
    {   // the root has no box of its own: the union of its children's
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 4; ++k) {
            if (bb.nodes4q[0].child[k] == PPG_BVH4_EMPTY) continue;
            float l[3], h[3];
            decodeChildBox(bb.nodes4q[0], k, l, h);
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], l[a]); hi[a] = std::max(hi[a], h[a]); }
        }
        rootArea = areaOf(lo, hi);
    }
    const double inv = rootArea > 0 ? 1.0 / rootArea : 0.0;
    std::vector<std::pair<int, uint32_t>> stack(1, {0, 1u});
    while (!stack.empty()) {
        const std::pair<int, uint32_t> e = stack.back();
        stack.pop_back();
        out->depth = std::max(out->depth, e.second);
        const Bvh4QNode &q = bb.nodes4q[(size_t)e.first];
        for (int k = 0; k < 4; ++k) {
            if (q.child[k] == PPG_BVH4_EMPTY) continue;
            float l[3], h[3];
            decodeChildBox(q, k, l, h);
            const double a = areaOf(l, h) * inv;
            if (q.child[k] >= 0) { out->sa_interior += a; stack.push_back({q.child[k], e.second + 1}); }
            else {
                const int cnt = (~q.child[k] & 7) + 1;
                out->sa_leaf += a; out->sa_tris += a * cnt; out->n_leaves++; out->leaf_hist[cnt]++;
            }
        }
    }
    return PPG_OK;
}
int ppg_debug_bvh_trace(const float *positions, const uint32_t *indices, uint32_t n_triangles, float pad_abs, int32_t max_leaf, const float *rays,
                        uint32_t n_rays, float *t_out, int32_t *orig_out, uint32_t *steps_out, uint32_t *tests_out, uint32_t *max_stack) {
    if (!positions || !indices || n_triangles == 0 || (n_rays && !rays)) return PPG_ERR_INVALID;
    BvhBuilder bb;
    bb.maxLeaf = std::max(1, std::min(8, (int)max_leaf));
    bb.run(positions, indices, n_triangles, pad_abs);
    std::vector<float4> accel(3 * (size_t)n_triangles);
    for (uint32_t k = 0; k < n_triangles; ++k) {
        const uint32_t t = bb.order[k];
        triAccelLoad(positions + 3 * indices[3 * t], positions + 3 * indices[3 * t + 1], positions + 3 * indices[3 * t + 2], (int)t, &accel[3 * (size_t)k]);
    }
    auto bits = [](unsigned int u) { float f; memcpy(&f, &u, 4); return f; };
    uint32_t deepest = 0;
    std::vector<int> stack;
    for (uint32_t r = 0; r < n_rays; ++r) {
        const float *R = rays + 8 * (size_t)r;
        const float o[3] = {R[0], R[1], R[2]}, d[3] = {R[4], R[5], R[6]}, mint = R[3], maxt = R[7];
        const float id[3] = {d[0] == 0.0f ? 1e30f : 1.0f / d[0], d[1] == 0.0f ? 1e30f : 1.0f / d[1], d[2] == 0.0f ? 1e30f : 1.0f / d[2]};  // safe_inv
        float bestT = INFINITY;
        int bestOrig = 0x7fffffff;
        bool found = false;
        uint32_t steps = 0, tests = 0;
        stack.clear();
        int cur = 0;
        for (;;) {
            if (cur >= 0) {  // bvh4_children
                ++steps;
                const Bvh4QNode &q = bb.nodes4q[(size_t)cur];
                const float tlim = std::min(maxt, bestT);
                const float org[3] = {q.ox, q.oy, q.oz};
                const unsigned int ql[3] = {q.qlox, q.qloy, q.qloz}, qh[3] = {q.qhix, q.qhiy, q.qhiz};
                float os[3], ids[3];
                for (int a = 0; a < 3; ++a) {
                    const unsigned int e = (q.exps >> (8 * a)) & 255u;
                    os[a] = (o[a] - org[a]) * bits((254u - e) << 23);
                    ids[a] = id[a] * bits(e << 23);
                }
                float ts[4]; int cs[4], m = 0;
                for (int k = 0; k < 4; ++k) {
                    float n = mint, f = INFINITY;
                    for (int a = 0; a < 3; ++a) {
                        const float lo = (float)((ql[a] >> (8 * k)) & 255u), hi = (float)((qh[a] >> (8 * k)) & 255u);
                        const float tn = ((id[a] < 0 ? hi : lo) - os[a]) * ids[a], tf = ((id[a] < 0 ? lo : hi) - os[a]) * ids[a];
                        n = std::max(n, tn); f = std::min(f, tf);
                    }
                    f = std::min(f * 1.0000008f, tlim);
                    const bool hit = n <= f && q.child[k] != PPG_BVH4_EMPTY;
                    ts[k] = hit ? n : INFINITY; cs[k] = q.child[k];
                    m += hit ? 1 : 0;
                }
                auto cswap = [&](int i, int j) { if (ts[i] > ts[j]) { std::swap(ts[i], ts[j]); std::swap(cs[i], cs[j]); } };
                cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
                if (m > 0) {
                    for (int k = m - 1; k >= 1; --k) stack.push_back(cs[k]);
                    deepest = std::max<uint32_t>(deepest, (uint32_t)stack.size());
                    cur = cs[0];
                    continue;
                }
            } else {  // leaf: tri_hit_regs on every triangle
                const int code = ~cur, first = code >> 3, cnt = (code & 7) + 1;
                for (int qd = first; qd < first + cnt; ++qd) {
                    ++tests;
                    const float4 a0 = accel[3 * (size_t)qd], a1 = accel[3 * (size_t)qd + 1], a2 = accel[3 * (size_t)qd + 2];
                    int k; memcpy(&k, &a0.w, 4);
                    if ((unsigned int)k > 2u) continue;
                    const bool k0 = k == 0, k1 = k == 1;
                    const float o_u = k0 ? o[1] : (k1 ? o[2] : o[0]), o_v = k0 ? o[2] : (k1 ? o[0] : o[1]), o_k = k0 ? o[0] : (k1 ? o[1] : o[2]);
                    const float d_u = k0 ? d[1] : (k1 ? d[2] : d[0]), d_v = k0 ? d[2] : (k1 ? d[0] : d[1]), d_k = k0 ? d[0] : (k1 ? d[1] : d[2]);
                    const float t = (a0.z - o_u * a0.x - o_v * a0.y - o_k) / (d_u * a0.x + d_v * a0.y + d_k);
                    if (t < mint || t > std::min(maxt, bestT)) continue;
                    const float hu = o_u + t * d_u - a1.x, hv = o_v + t * d_v - a1.y;
                    const float u = hv * a1.z + hu * a1.w, v = hu * a2.x + hv * a2.y;
                    if (!(u >= 0 && v >= 0 && u + v <= 1.0f)) continue;
                    int orig; memcpy(&orig, &a2.w, 4);
                    if (!found || t < bestT || (t == bestT && orig < bestOrig)) { bestT = t; bestOrig = orig; found = true; }
                }
            }
            if (stack.empty()) break;
            cur = stack.back();
            stack.pop_back();
        }
        if (t_out) t_out[r] = found ? bestT : INFINITY;
        if (orig_out) orig_out[r] = found ? bestOrig : -1;
        if (steps_out) steps_out[r] = steps;
        if (tests_out) tests_out[r] = tests;
    }
    if (max_stack) *max_stack = deepest;
    return PPG_OK;
}
// ReconstructionFilter::configure (rfilter.cpp:37-55) with the eval() of src/rfilters/*.cpp, in the reference's float arithmetic
static int rfilterTable(const ppg_rfilter *f, float table[32], float *radius, int32_t *border, std::string &err) {
    const int type = f->type;
    float r = 0.0f;
    switch (type) {
    case PPG_RFILTER_BOX:
        if (!(std::isfinite(f->radius) && f->radius > 0.0f)) { err = "box filter: radius must be positive"; return PPG_ERR_INVALID; }
        r = f->radius + 1e-5f; break;                                                        // box.cpp
    case PPG_RFILTER_TENT: r = 1.0f; break;                                                  // tent.cpp
    case PPG_RFILTER_GAUSSIAN:
        if (!(std::isfinite(f->stddev) && f->stddev > 0.0f)) { err = "gaussian filter: stddev must be positive"; return PPG_ERR_INVALID; }
        r = 4 * f->stddev; break;                                                            // gaussian.cpp
    case PPG_RFILTER_MITCHELL:
        if (!(std::isfinite(f->B) && std::isfinite(f->C))) { err = "mitchell filter: B and C must be finite"; return PPG_ERR_INVALID; }
        r = 2.0f; break;                                                                     // mitchell.cpp
    case PPG_RFILTER_CATMULLROM: r = 2.0f; break;                                            // catmullrom.cpp
    case PPG_RFILTER_LANCZOS:
        if (f->lobes < 1) { err = "lanczos filter: lobes must be >= 1"; return PPG_ERR_INVALID; }
        r = (float)f->lobes; break;                                                          // lanczos.cpp
    default: err = "unknown reconstruction filter type"; return PPG_ERR_INVALID;
    }
    const float stddev = f->stddev, B = f->B, C = f->C;
    auto mitchell = [](float x, float B, float C) {
        x = std::fabs(x);
        const float x2 = x * x, x3 = x2 * x;
        if (x < 1) return 1.0f / 6.0f * ((12 - 9 * B - 6 * C) * x3 + (-18 + 12 * B + 6 * C) * x2 + (6 - 2 * B));
        if (x < 2) return 1.0f / 6.0f * ((-B - 6 * C) * x3 + (6 * B + 30 * C) * x2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C));
        return 0.0f;
    };
    auto eval = [&](float x) -> float {
        switch (type) {
        case PPG_RFILTER_BOX: return std::fabs(x) <= r ? 1.0f : 0.0f;
        case PPG_RFILTER_TENT: return std::max(0.0f, 1.0f - std::fabs(x / r));
        case PPG_RFILTER_GAUSSIAN: {
            const float alpha = -1.0f / (2.0f * stddev * stddev);  // math::fastexp: (float) exp((double) x)
            return std::max(0.0f, (float)std::exp((double)(alpha * x * x)) - (float)std::exp((double)(alpha * r * r)));
        }
        case PPG_RFILTER_MITCHELL: return mitchell(x, B, C);
        case PPG_RFILTER_CATMULLROM: return mitchell(x, 0.0f, 0.5f);
        default: {
            x = std::fabs(x);
            if (x < 1e-4f) return 1.0f;  // Epsilon (single precision)
            if (x > r) return 0.0f;
            const float x1 = (float)(M_PI * (double)x), x2 = x1 / r;
            return (std::sin(x1) * std::sin(x2)) / (x1 * x2);
        }
        }
    };
    float sum = 0.0f;
    for (int i = 0; i < 31; ++i) { table[i] = eval((r * (float)i) / 31); sum += table[i]; }
    table[31] = 0.0f;
    sum *= 2 * r / 31;
    const float normalization = 1.0f / sum;
    for (int i = 0; i < 31; ++i) table[i] *= normalization;
    *radius = r;
    *border = (int32_t)std::ceil(r - 0.5f);
    if (!std::isfinite(normalization)) { err = "reconstruction filter: its samples sum to zero"; return PPG_ERR_INVALID; }
    if (*border > PPG_RFILTER_MAX_BORDER) { err = "reconstruction filter: radius too large (border > 3, more than 7x7 pixels per sample)"; return PPG_ERR_INVALID; }
    return PPG_OK;
}

void ppg_rfilter_default(ppg_rfilter *f) {
    f->type = PPG_RFILTER_BOX; f->radius = 0.5f; f->stddev = 0.5f; f->B = 1.0f / 3.0f; f->C = 1.0f / 3.0f; f->lobes = 3;
}

int ppg_set_rfilter(ppg_ctx *ctx, const ppg_rfilter *f) {
    ppg_rfilter d;
    ppg_rfilter_default(&d);
    if (!f) f = &d;
    float table[32], r = 0.0f;
    int32_t border = 0;
    std::string err;
    if (int rc = rfilterTable(f, table, &r, &border, err)) { ctx->error = err; return rc; }
    const bool filtered = !(f->type == PPG_RFILTER_BOX && f->radius == 0.5f);
    if (filtered && ctx->shardWorld > 1 && !ctx->footHook) { ctx->error = kShardedFilter; return PPG_ERR_INVALID; }
    ctx->filtered = filtered;
    ctx->rfBorder = border;
    memcpy(ctx->rf.table, table, sizeof table);
    ctx->rf.radius = r; ctx->rf.scale = 31 / r;  // m_scaleFactor = MTS_FILTER_RESOLUTION / m_radius
    return PPG_OK;
}

int ppg_set_lens(ppg_ctx *ctx, const ppg_lens *lens) {
    if (lens && !(std::isfinite(lens->aperture_radius) && lens->aperture_radius > 0)) { ctx->error = "thin lens: aperture_radius must be finite and > 0"; return PPG_ERR_INVALID; }
    if (lens && !(std::isfinite(lens->focus_distance) && lens->focus_distance > 0)) { ctx->error = "thin lens: focus_distance must be finite and > 0"; return PPG_ERR_INVALID; }
    (void)hipSetDevice(ctx->device);
    ctx->quiesce();
    ctx->lensOn = lens != nullptr;
    ctx->lens = lens ? *lens : ppg_lens{};
    DevScene &S = ctx->scene;
    S.cam.lens = ctx->lensOn ? 1 : 0; S.cam.aperture = ctx->lens.aperture_radius; S.cam.focus = ctx->lens.focus_distance;
    if (ctx->haveScene) {  // the scene's box and what depends on it, with the new sensor box (and the delta emitters the scene was built with)
        const SceneBox box = sceneBox(ctx->geomMin, ctx->geomMax, ctx->lensOn ? &ctx->lens : nullptr, S.cam.c2w, ctx->sceneDelta);
        for (int a = 0; a < 3; ++a) { ctx->aabbMin[a] = box.mn[a]; ctx->aabbMax[a] = box.mx[a]; }
        if (S.env.w != 0) S.bsphere = envBSphere(ctx->aabbMin, ctx->aabbMax);
    }
    return PPG_OK;
}

int ppg_set_material_textures(ppg_ctx *ctx, const ppg_material_textures *slots, uint32_t n) { return setSideList(ctx, "material textures", ctx->materialTextures, slots, n, false); }
int ppg_set_microfacet(ppg_ctx *ctx, const ppg_microfacet *m, uint32_t n) { return setSideList(ctx, "microfacet", ctx->microfacet, m, n, true); }
int ppg_set_coatings(ppg_ctx *ctx, const ppg_coating *c, uint32_t n) { return setSideList(ctx, "coatings", ctx->coatings, c, n, true); }
int ppg_set_blends(ppg_ctx *ctx, const ppg_blend *b, uint32_t n) { return setSideList(ctx, "blends", ctx->blends, b, n, true); }

int ppg_set_delta_emitters(ppg_ctx *ctx, const ppg_delta_emitter *em, uint32_t n) {
    if (ctx->renderOpen) { ctx->error = "delta emitters: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && !em) { ctx->error = "delta emitters: no list"; return PPG_ERR_INVALID; }
    auto finite = [](const float *v, int k) { for (int i = 0; i < k; ++i) if (!std::isfinite(v[i])) return false; return true; };
    for (uint32_t k = 0; k < n; ++k) {
        const ppg_delta_emitter &e = em[k];
        const std::string who = "delta emitter " + std::to_string(k) + ": ";
        if (e.type != PPG_EMITTER_POINT && e.type != PPG_EMITTER_SPOT && e.type != PPG_EMITTER_DIRECTIONAL) { ctx->error = who + "unknown type"; return PPG_ERR_INVALID; }
        if (!finite(e.intensity, 3) || !finite(e.position, 3) || !finite(e.to_local, 9) || !finite(e.direction, 3) || !std::isfinite(e.cutoff_angle) ||
            !std::isfinite(e.beam_width)) { ctx->error = who + "a value is not finite"; return PPG_ERR_INVALID; }
        if (e.intensity[0] < 0 || e.intensity[1] < 0 || e.intensity[2] < 0) { ctx->error = who + "negative intensity"; return PPG_ERR_INVALID; }
        if (e.type == PPG_EMITTER_SPOT && !(0 < e.beam_width && e.beam_width <= e.cutoff_angle && e.cutoff_angle < 0.5f * PPG_PI_F)) {
            ctx->error = who + "spot angles must satisfy 0 < beam_width <= cutoff_angle < pi/2"; return PPG_ERR_INVALID;
        }
        if (e.type == PPG_EMITTER_DIRECTIONAL && e.direction[0] == 0 && e.direction[1] == 0 && e.direction[2] == 0) { ctx->error = who + "zero direction"; return PPG_ERR_INVALID; }
    }
    ctx->deltaEmitters.assign(em, em + n);
    return PPG_OK;
}

int ppg_set_media(ppg_ctx *ctx, const ppg_media *media) {
    if (ctx->renderOpen) { ctx->error = "media: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (media && media->n_media && !media->media) { ctx->error = "media: n_media > 0 but no array"; return PPG_ERR_INVALID; }  // (the kept list stays)
    ctx->mediaList = ppg_media{};
    ctx->media.clear(); ctx->triMedia.clear(); ctx->sphereMedia.clear(); ctx->shapeMedia.clear();
    if (!media || media->n_media == 0) return PPG_OK;  // cleared
    // the list is copied as it is and validated against the scene by ppg_set_scene
    ctx->media.assign(media->media, media->media + media->n_media);
    if (media->tri_media) ctx->triMedia.assign(media->tri_media, media->tri_media + media->n_tri_media);
    if (media->sphere_media) ctx->sphereMedia.assign(media->sphere_media, media->sphere_media + media->n_sphere_media);
    if (media->shape_media) ctx->shapeMedia.assign(media->shape_media, media->shape_media + media->n_shape_media);
    ppg_media &L = ctx->mediaList;
    L = *media;
    L.media = ctx->media.data();
    // (an array of no entries is still an array: its count is checked against the scene's)
    static const uint32_t none = 0;
    L.tri_media = media->tri_media ? (ctx->triMedia.empty() ? &none : ctx->triMedia.data()) : nullptr;
    L.sphere_media = media->sphere_media ? (ctx->sphereMedia.empty() ? &none : ctx->sphereMedia.data()) : nullptr;
    L.shape_media = media->shape_media ? (ctx->shapeMedia.empty() ? &none : ctx->shapeMedia.data()) : nullptr;
    return PPG_OK;
}

int ppg_set_media_volumes(ppg_ctx *ctx, const ppg_media_volumes *volumes) {
    if (ctx->renderOpen) { ctx->error = "media volumes: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (volumes && volumes->n_entries) {  // (what cannot even be copied is refused here; the kept list stays)
        if (!volumes->entries || (volumes->n_volumes && !volumes->volumes)) { ctx->error = "media volumes: a count > 0 but no array"; return PPG_ERR_INVALID; }
        for (uint32_t k = 0; k < volumes->n_volumes; ++k) {
            const ppg_volume &v = volumes->volumes[k];
            if (v.kind != PPG_VOLUME_GRID) continue;
            const std::string who = "media volumes: volume " + std::to_string(k) + ": ";
            if (v.channels != 1 && v.channels != 3) { ctx->error = who + "channels must be 1 or 3"; return PPG_ERR_INVALID; }
            for (int a = 0; a < 3; ++a) if (v.res[a] < 2) { ctx->error = who + "a res component is below 2"; return PPG_ERR_INVALID; }
            if ((double)v.res[0] * v.res[1] * v.res[2] * v.channels > 536870912.0) { ctx->error = who + "more than 2^29 floats"; return PPG_ERR_INVALID; }
            if (!v.data) { ctx->error = who + "a grid without data"; return PPG_ERR_INVALID; }
        }
    }
    ctx->volumesList = ppg_media_volumes{};
    ctx->volumes.clear(); ctx->volumeData.clear(); ctx->volumeEntries.clear();
    if (!volumes || volumes->n_entries == 0) return PPG_OK;  // cleared
    // the list is copied as it is, the grids' data with it, and validated against the media list by ppg_set_scene
    ctx->volumes.assign(volumes->volumes, volumes->volumes + volumes->n_volumes);
    ctx->volumeEntries.assign(volumes->entries, volumes->entries + volumes->n_entries);
    ctx->volumeData.resize(volumes->n_volumes);
    for (uint32_t k = 0; k < volumes->n_volumes; ++k) {
        ppg_volume &v = ctx->volumes[k];
        if (v.kind != PPG_VOLUME_GRID) { v.data = nullptr; continue; }
        const size_t count = (size_t)v.res[0] * v.res[1] * v.res[2] * v.channels;
        ctx->volumeData[k].assign(v.data, v.data + count);
        v.data = ctx->volumeData[k].data();
    }
    ppg_media_volumes &L = ctx->volumesList;
    L = *volumes;
    L.volumes = ctx->volumes.data();
    L.entries = ctx->volumeEntries.data();
    return PPG_OK;
}

int ppg_set_shapes(ppg_ctx *ctx, const ppg_shape *shapes, uint32_t n) {
    if (ctx->renderOpen) { ctx->error = "shapes: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && !shapes) { ctx->error = "shapes: no list"; return PPG_ERR_INVALID; }
    ctx->shapes.assign(shapes, shapes + n);  // validated against the scene by ppg_set_scene
    return PPG_OK;
}

// ---- include/ppg_testhooks.h: the render's own device functions, one item per lane (the kernels: ppg_inst.hip, the shapes unit) ----
struct DebugBuf {  // a device array for the length of one hook call
    void *p = nullptr;
    ~DebugBuf() { if (p) (void)hipFree(p); }
    hipError_t fill(const void *src, size_t bytes) {
        hipError_t e = hipMalloc(&p, std::max<size_t>(16, bytes));
        if (e == hipSuccess && src && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        return e;
    }
};
int ppg_debug_intersect(ppg_ctx *ctx, uint32_t n, const float *rays, ppg_debug_hit *out, int32_t any_hit) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_intersect: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && (!rays || !out)) { ctx->error = "ppg_debug_intersect: no arrays"; return PPG_ERR_INVALID; }
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dRays, dOut;
    HIP_CHECK(dRays.fill(rays, 2 * (size_t)n * sizeof(float4)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_hit)));
    const unsigned int block = 64;
    launcher(ppg_path_kernels[PPG_FAMILY_SHAPES].debug_intersect)((int)((n + block - 1) / block), (int)block, ctx->stream, ctx->scene, n, (const float4 *)dRays.p, (ppg_debug_hit *)dOut.p, any_hit ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_hit), hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_debug_medium(ppg_ctx *ctx, uint32_t n, const ppg_debug_medium_item *items, ppg_debug_medium_out *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_medium: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (!ctx->mediaArgs.media) { ctx->error = "ppg_debug_medium: the scene binds no medium"; return PPG_ERR_STATE; }
    if (n && (!items || !out)) { ctx->error = "ppg_debug_medium: no arrays"; return PPG_ERR_INVALID; }
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].medium < 0 || items[i].medium >= ctx->mediaArgs.n_media) { ctx->error = "ppg_debug_medium: item " + std::to_string(i) + ": medium out of range"; return PPG_ERR_INVALID; }
        for (int k = 0; k < 4; ++k)
            if (!(items[i].u[k] >= 0.0f && items[i].u[k] <= 1.0f)) { ctx->error = "ppg_debug_medium: item " + std::to_string(i) + ": a sample outside [0, 1]"; return PPG_ERR_INVALID; }
    }
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dItems, dOut;
    HIP_CHECK(dItems.fill(items, (size_t)n * sizeof(ppg_debug_medium_item)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_medium_out)));
    const unsigned int block = 64;
    launcher(ppg_path_kernels[PPG_FAMILY_MEDIA].debug_medium)((int)((n + block - 1) / block), (int)block, ctx->stream, ctx->mediaArgs, n, (const ppg_debug_medium_item *)dItems.p,
                                                              (ppg_debug_medium_out *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_medium_out), hipMemcpyDeviceToHost));
    return PPG_OK;
}
// ppg_debug_volume, ppg_debug_hetmedium: what both refuse, then upload, launch and read back
extern "C++" {
template <typename Item, typename Out, typename Launch>
static int debugHet(ppg_ctx *ctx, const char *who, uint32_t n, const Item *items, Out *out, Launch launch) {
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dItems, dOut;
    HIP_CHECK(dItems.fill(items, (size_t)n * sizeof(Item)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(Out)));
    const unsigned int block = 64;
    launch((int)((n + block - 1) / block), (int)block, (const Item *)dItems.p, (Out *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(Out), hipMemcpyDeviceToHost));
    return PPG_OK;
}
static int debugHetRefusal(ppg_ctx *ctx, const std::string &who, uint32_t n, const void *items, const void *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = who + ": not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (!ctx->hetArgs.het) { ctx->error = who + ": the scene binds no heterogeneous medium"; return PPG_ERR_STATE; }
    if (n && (!items || !out)) { ctx->error = who + ": no arrays"; return PPG_ERR_INVALID; }
    return PPG_OK;
}
}  // extern "C++"
int ppg_debug_volume(ppg_ctx *ctx, uint32_t n, const ppg_debug_volume_item *items, ppg_debug_volume_out *out) {
    if (int rc = debugHetRefusal(ctx, "ppg_debug_volume", n, items, out)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (items[i].volume < 0 || items[i].volume >= ctx->hetArgs.n_volumes) { ctx->error = "ppg_debug_volume: item " + std::to_string(i) + ": volume out of range"; return PPG_ERR_INVALID; }
    return debugHet(ctx, "ppg_debug_volume", n, items, out, [&](int grid, int block, const ppg_debug_volume_item *dIn, ppg_debug_volume_out *dOut) {
        launcher(ppg_path_kernels[PPG_FAMILY_HETMEDIA].debug_volume)(grid, block, ctx->stream, ctx->hetArgs, n, dIn, dOut);
    });
}
int ppg_debug_hetmedium(ppg_ctx *ctx, uint32_t n, const ppg_debug_hetmedium_item *items, ppg_debug_hetmedium_out *out) {
    if (int rc = debugHetRefusal(ctx, "ppg_debug_hetmedium", n, items, out)) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].medium < 0 || items[i].medium >= ctx->mediaArgs.n_media) { ctx->error = "ppg_debug_hetmedium: item " + std::to_string(i) + ": medium out of range"; return PPG_ERR_INVALID; }
        if (!ctx->hetMedium[items[i].medium]) { ctx->error = "ppg_debug_hetmedium: item " + std::to_string(i) + ": the medium is not heterogeneous"; return PPG_ERR_INVALID; }
    }
    return debugHet(ctx, "ppg_debug_hetmedium", n, items, out, [&](int grid, int block, const ppg_debug_hetmedium_item *dIn, ppg_debug_hetmedium_out *dOut) {
        launcher(ppg_path_kernels[PPG_FAMILY_HETMEDIA].debug_hetmedium)(grid, block, ctx->stream, ctx->hetArgs, n, dIn, dOut);
    });
}
int ppg_debug_shading_frame(ppg_ctx *ctx, uint32_t n, const float *rays, ppg_debug_frame *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_shading_frame: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && (!rays || !out)) { ctx->error = "ppg_debug_shading_frame: no arrays"; return PPG_ERR_INVALID; }
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dRays, dOut;
    HIP_CHECK(dRays.fill(rays, 2 * (size_t)n * sizeof(float4)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_frame)));
    const unsigned int block = 64;
    // (the top family compiles the hook's kernel, and every feature a scene may hold)
    launcher(ppg_path_kernels[PPG_FAMILY_LOBES].debug_shading_frame)((int)((n + block - 1) / block), (int)block, ctx->stream, ctx->scene, n, (const float4 *)dRays.p, (ppg_debug_frame *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_frame), hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_debug_camera_rays(ppg_ctx *ctx, uint32_t first_sample, uint32_t n_samples, float *rays) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_camera_rays: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n_samples && !rays) { ctx->error = "ppg_debug_camera_rays: no array"; return PPG_ERR_INVALID; }
    if (n_samples == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    const unsigned int nPix = (unsigned int)ctx->W * (unsigned int)ctx->H;
    const size_t bytes = 2 * (size_t)n_samples * nPix * sizeof(float4);
    DebugBuf dRays;
    HIP_CHECK(dRays.fill(nullptr, bytes));
    hipLaunchKernelGGL(k_debug_camera_rays, dim3((nPix + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->scene.cam, (unsigned long long)ctx->seed, first_sample, n_samples, nPix,
                       (float4 *)dRays.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(rays, dRays.p, bytes, hipMemcpyDeviceToHost));
    return PPG_OK;
}

// ---- include/ppg.h "Feature buffers of the first hit" ----
// the inverse of a row-major 4x4 in double (Gauss-Jordan with partial pivoting); false: singular
static bool invert4x4(const float *m, double inv[16]) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = (double)m[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int i = c + 1; i < 4; ++i) if (std::fabs(a[i][c]) > std::fabs(a[piv][c])) piv = i;
        if (!(std::fabs(a[piv][c]) > 0.0)) return false;
        if (piv != c) for (int j = 0; j < 8; ++j) std::swap(a[piv][j], a[c][j]);
        const double d = a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int i = 0; i < 4; ++i) {
            if (i == c) continue;
            const double f = a[i][c];
            if (f != 0.0) for (int j = 0; j < 8; ++j) a[i][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) inv[4 * i + j] = a[i][4 + j];
    return true;
}
int ppg_render_fields(ppg_ctx *ctx, const ppg_fields *f, float *out) {
    if (!ctx) return PPG_ERR_INVALID;
    if (!f || !out) { ctx->error = "ppg_render_fields: no fields or no output array"; return PPG_ERR_INVALID; }
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_render_fields: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (f->n_fields < 1 || f->n_fields > PPG_MAX_FIELDS) { ctx->error = "ppg_render_fields: n_fields must be 1 .. " + std::to_string(PPG_MAX_FIELDS); return PPG_ERR_INVALID; }
    FieldsRequest F{};
    F.n_fields = (int)f->n_fields;
    for (uint32_t k = 0; k < f->n_fields; ++k) {
        if (f->field[k] < PPG_FIELD_POSITION || f->field[k] > PPG_FIELD_PRIM_INDEX) {
            ctx->error = "ppg_render_fields: field " + std::to_string(k) + ": unknown field " + std::to_string(f->field[k]); return PPG_ERR_INVALID;
        }
        F.field[k] = f->field[k];
        memcpy(F.undefined[k], f->undefined[k], sizeof F.undefined[k]);
        if (f->field[k] == PPG_FIELD_ALBEDO) F.albedo = 1;
    }
    if (f->spp < 1 || f->spp > 65536) { ctx->error = "ppg_render_fields: spp must be 1 .. 65536"; return PPG_ERR_INVALID; }
    if (F.albedo && ctx->scene.blend) { ctx->error = "albedo: blendbsdf / mixturebsdf materials are not supported yet"; return PPG_ERR_INVALID; }
    double inv[16];
    if (!invert4x4(ctx->scene.cam.c2w, inv)) { ctx->error = "ppg_render_fields: camera_to_world is not invertible"; return PPG_ERR_INVALID; }
    for (int i = 0; i < 16; ++i) F.w2c[i] = (float)inv[i];
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    const size_t n = (size_t)ctx->W * (size_t)ctx->H, planes = (size_t)f->n_fields * 3 * n;
    // what multiplies a material's diffuse reflectance: 1 - fdrExt of a plastic (plastic.cpp:195, 219-221), 0 where there is no diffuse reflection
    std::vector<float> scale(std::max<uint32_t>(1u, ctx->nMaterials), 0.0f);
    if (F.albedo && ctx->nMaterials) {
        std::vector<float4> mats(PPG_MAT_STRIDE * (size_t)ctx->nMaterials);
        HIP_CHECK(hipMemcpy(mats.data(), ctx->scene.materials, mats.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < ctx->nMaterials; ++i) {
            const int type = (int)mats[PPG_MAT_STRIDE * (size_t)i].w;
            if (type == PPG_BSDF_DIFFUSE || type == PPG_BSDF_TWOSIDED_DIFFUSE || type == PPG_BSDF_ROUGHDIFFUSE || type == PPG_BSDF_PHONG || type == PPG_BSDF_ROUGHPLASTIC) scale[i] = 1.0f;
            else if (type == PPG_BSDF_PLASTIC) scale[i] = 1 - ppg_fresnel_diffuse_reflectance(mats[PPG_MAT_STRIDE * (size_t)i + 2].x);
        }
    }
    DebugBuf dScale, dVals, dPos, dSum, dW, dOut;
    HIP_CHECK(dScale.fill(scale.data(), scale.size() * sizeof(float)));
    HIP_CHECK(dVals.fill(nullptr, planes * sizeof(float)));
    HIP_CHECK(dPos.fill(nullptr, 2 * n * sizeof(float)));
    HIP_CHECK(dSum.fill(nullptr, planes * sizeof(float)));
    HIP_CHECK(dW.fill(nullptr, n * sizeof(float)));
    HIP_CHECK(dOut.fill(nullptr, planes * sizeof(float)));
    HIP_CHECK(hipMemsetAsync(dSum.p, 0, planes * sizeof(float), ctx->stream));
    HIP_CHECK(hipMemsetAsync(dW.p, 0, n * sizeof(float), ctx->stream));
    // (the top family compiles the kernels, and every feature a scene may hold)
    const PathKernels &K = ppg_path_kernels[PPG_FAMILY_LOBES];
    FieldsSampleLaunch s{ctx->stream, ctx->scene, F, (unsigned long long)ctx->seed, 0u, (const float *)dScale.p, (float *)dVals.p, (float *)dPos.p};
    FieldsResolveLaunch r{ctx->stream, ctx->rf, ctx->rfBorder, F.n_fields, (const float *)dVals.p, (const float *)dPos.p, (float *)dSum.p, (float *)dW.p};
    r.ff.W = ctx->W; r.ff.H = ctx->H;
    if (!ctx->filtered) {  // the default box: the sample's own pixel with weight 1, as k_film has it
        for (float &t : r.ff.table) t = 1.0f;
        r.ff.radius = 0.5f; r.ff.scale = 62.0f; r.border = 0;
    }
    for (uint32_t j = 0; j < f->spp; ++j) {
        s.sample = f->first_sample + j;
        launcher(K.fields_sample)(s);
        launcher(K.fields_resolve)(r);
    }
    for (uint32_t k = 0; k < f->n_fields; ++k)
        hipLaunchKernelGGL(k_normalise, dim3(((unsigned int)n + 255) / 256), dim3(256), 0, ctx->stream, (int)n, (const float *)dSum.p + (size_t)k * 3 * n, (const float *)dW.p,
                           (float *)dOut.p + (size_t)k * 3 * n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, planes * sizeof(float), hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_debug_intersect_mode(ppg_ctx *ctx, uint32_t n, const float *rays, ppg_debug_hit *out, int32_t mode, int32_t param, uint32_t *stats_out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_intersect_mode: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && (!rays || !out)) { ctx->error = "ppg_debug_intersect_mode: no arrays"; return PPG_ERR_INVALID; }
    if (mode < PPG_DEBUG_TRACE_LANE || mode > PPG_DEBUG_TRACE_KTRACE || param < 0) { ctx->error = "ppg_debug_intersect_mode: no such mode or a negative parameter"; return PPG_ERR_INVALID; }
    if (mode == PPG_DEBUG_TRACE_LANE_VOTE && n % 64u) { ctx->error = "ppg_debug_intersect_mode: the leaf vote runs whole waves, n must be a multiple of 64"; return PPG_ERR_INVALID; }
    if (mode == PPG_DEBUG_TRACE_RESUME && param > 31) { ctx->error = "ppg_debug_intersect_mode: suspend_lanes above 31"; return PPG_ERR_INVALID; }
    if (stats_out) memset(stats_out, 0, 4 * sizeof(uint32_t));
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dRays, dOut, dStats;
    HIP_CHECK(dRays.fill(rays, 2 * (size_t)n * sizeof(float4)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_hit)));
    HIP_CHECK(dStats.fill(nullptr, 4 * sizeof(uint32_t)));
    HIP_CHECK(hipMemsetAsync(dStats.p, 0, 4 * sizeof(uint32_t), ctx->stream));
    const PathKernels &K = ppg_path_kernels[PPG_FAMILY_SHAPES];
    if (mode != PPG_DEBUG_TRACE_KTRACE) {
        launcher(K.debug_trace)(mode, param, ctx->stream, ctx->scene, n, (const float4 *)dRays.p, (ppg_debug_hit *)dOut.p, (unsigned int *)dStats.p);
    } else {
        // the rays as the paths of a batch: k_trace at a first bounce reads ray_o / ray_d of every path and writes hit (renderBatch)
        const int grid = param > 0 ? std::min(param, 4096) : (int)((n + 1023u) / 1024u);
        DebugBuf dO, dD, dHit, dBlock;
        std::vector<float4> ro(n), rd(n);
        for (uint32_t i = 0; i < n; ++i) {
            const float *r = rays + 8 * (size_t)i;
            ro[i] = make_float4(r[0], r[1], r[2], r[3]); rd[i] = make_float4(r[4], r[5], r[6], r[7]);
        }
        HIP_CHECK(dO.fill(ro.data(), (size_t)n * sizeof(float4)));
        HIP_CHECK(dD.fill(rd.data(), (size_t)n * sizeof(float4)));
        HIP_CHECK(dHit.fill(nullptr, (size_t)n * sizeof(float4)));
        HIP_CHECK(dBlock.fill(nullptr, (size_t)grid * sizeof(BlockStats)));
        HIP_CHECK(hipMemsetAsync(dHit.p, 0xff, (size_t)n * sizeof(float4), ctx->stream));  // (prim -1 wherever k_trace writes nothing)
        HIP_CHECK(hipMemsetAsync(dBlock.p, 0, (size_t)grid * sizeof(BlockStats), ctx->stream));
        PathState P{};
        P.n_paths = n; P.n_pix = n;
        P.ray_o = {(float4 *)dO.p, 1u}; P.ray_d = {(float4 *)dD.p, 1u}; P.hit = {(float4 *)dHit.p, 1u};
        Queues Q{};
        Q.cap = n; Q.n_blocks = (unsigned int)grid; Q.stats = (BlockStats *)dBlock.p;
        const bool smallScene = isSmallScene(ctx);
        const size_t traceLds = smallScene ? (size_t)ctx->ldsTris * 48 : (size_t)PPG_TRACE_STACK * PPG_BLOCK * 4 + (PPG_BLOCK / 64) * sizeof(PairLds);
        TraceLaunch a{grid, traceLds, ctx->stream, P, ctx->scene, Q, QIN_FIRST, smallScene ? 0 : ctx->ldsNodes, ctx->ldsTris, nullptr, nullptr, smallScene, false};
        launcher(ppg_path_kernels[sceneFamily(ctx->scene, ctx->mediaArgs, ctx->hetArgs)].trace)(a);
        HIP_CHECK(hipGetLastError());
        launcher(K.debug_hit_records)(ctx->stream, ctx->scene, n, (const float4 *)dRays.p, (const float4 *)dHit.p, (ppg_debug_hit *)dOut.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (the buffers of this branch go out of scope)
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_hit), hipMemcpyDeviceToHost));
    if (stats_out) {
        HIP_CHECK(hipMemcpy(stats_out, dStats.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        stats_out[2] = (uint32_t)ctx->scene.n_top;
        stats_out[3] = mode == PPG_DEBUG_TRACE_KTRACE && isSmallScene(ctx) ? 1u : 0u;
    }
    return PPG_OK;
}
// emitter_sample_direct<full> of kernel family `family` (both checked by the caller).  A sample outside [0, 1] is refused: beyond 1 pmf_sample's
// forward skip can leave the emitter's tables (include/ppg_testhooks.h).
static int debugSampleDirect(ppg_ctx *ctx, const char *who, int family, int full, uint32_t n, const float *ref, const float *ref_n, const float *u, ppg_debug_direct_ex *out) {
    if (n && (!ref || !ref_n || !u || !out)) { ctx->error = std::string(who) + ": no arrays"; return PPG_ERR_INVALID; }
    for (uint32_t i = 0; i < n; ++i)
        if (!(u[2 * i] >= 0.0f && u[2 * i] <= 1.0f && u[2 * i + 1] >= 0.0f && u[2 * i + 1] <= 1.0f)) { ctx->error = std::string(who) + ": item " + std::to_string(i) + ": a sample outside [0, 1]"; return PPG_ERR_INVALID; }
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dRef, dRefN, dU, dOut;
    HIP_CHECK(dRef.fill(ref, 3 * (size_t)n * sizeof(float)));
    HIP_CHECK(dRefN.fill(ref_n, 3 * (size_t)n * sizeof(float)));
    HIP_CHECK(dU.fill(u, 2 * (size_t)n * sizeof(float)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_direct_ex)));
    const unsigned int block = 64;
    launcher(ppg_path_kernels[family].debug_sample_direct)(full, (int)((n + block - 1) / block), (int)block, ctx->stream, ctx->scene, n, (const float *)dRef.p,
                                                           (const float *)dRefN.p, (const float *)dU.p, (ppg_debug_direct_ex *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_direct_ex), hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_debug_sample_direct(ppg_ctx *ctx, uint32_t n, const float *ref, const float *ref_n, const float *u, ppg_debug_direct *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_sample_direct: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (n && !out) { ctx->error = "ppg_debug_sample_direct: no arrays"; return PPG_ERR_INVALID; }
    std::vector<ppg_debug_direct_ex> ex(n);
    if (const int rc = debugSampleDirect(ctx, "ppg_debug_sample_direct", PPG_FAMILY_SHAPES, 1, n, ref, ref_n, u, ex.data())) return rc;
    static_assert(offsetof(ppg_debug_direct, _pad) == offsetof(ppg_debug_direct_ex, sd), "the extended record starts with the plain one");
    for (uint32_t i = 0; i < n; ++i) {  // the plain record: the extended one's first 52 bytes, the padding 0
        memset(&out[i], 0, sizeof out[i]);
        memcpy(&out[i], &ex[i], offsetof(ppg_debug_direct, _pad));
    }
    return PPG_OK;
}
// a kernel family can read the scene if it is the scene's own or one above it (every family knows what the families below it know)
static int debugFamily(ppg_ctx *ctx, const char *who, int32_t family, int *out) {
    const int own = sceneFamily(ctx->scene, ctx->mediaArgs, ctx->hetArgs);
    if (family < -1 || family >= PPG_DEBUG_FAMILIES) { ctx->error = std::string(who) + ": no such kernel family"; return PPG_ERR_INVALID; }
    if (family >= 0 && family < own) { ctx->error = std::string(who) + ": the scene needs kernel family " + std::to_string(own) + " or above"; return PPG_ERR_INVALID; }
    *out = family < 0 ? own : family;
    return PPG_OK;
}
int ppg_debug_sample_direct_as(ppg_ctx *ctx, int32_t family, int32_t full, uint32_t n, const float *ref, const float *ref_n, const float *u, ppg_debug_direct_ex *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_sample_direct_as: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    int fam = 0;
    if (const int rc = debugFamily(ctx, "ppg_debug_sample_direct_as", family, &fam)) return rc;
    if (family < 0) full = ctx->fullMaterials ? 1 : 0;
    if (!full && fam != PPG_FAMILY_BASE) { ctx->error = "ppg_debug_sample_direct_as: full = 0 exists in the base family only"; return PPG_ERR_INVALID; }
    if (!full && ctx->fullMaterials) { ctx->error = "ppg_debug_sample_direct_as: the scene needs the FULL kernels"; return PPG_ERR_INVALID; }
    return debugSampleDirect(ctx, "ppg_debug_sample_direct_as", fam, full ? 1 : 0, n, ref, ref_n, u, out);
}
int ppg_debug_pdf_direct(ppg_ctx *ctx, int32_t family, uint32_t n, const float *rays, const float *ref_n, ppg_debug_pdf *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_pdf_direct: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    int fam = 0;
    if (const int rc = debugFamily(ctx, "ppg_debug_pdf_direct", family, &fam)) return rc;
    if (n && (!rays || !ref_n || !out)) { ctx->error = "ppg_debug_pdf_direct: no arrays"; return PPG_ERR_INVALID; }
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dRays, dRefN, dOut;
    HIP_CHECK(dRays.fill(rays, 2 * (size_t)n * sizeof(float4)));
    HIP_CHECK(dRefN.fill(ref_n, 3 * (size_t)n * sizeof(float)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_pdf)));
    const unsigned int block = 64;
    launcher(ppg_path_kernels[fam].debug_pdf_direct)((int)((n + block - 1) / block), (int)block, ctx->stream, ctx->scene, n, (const float4 *)dRays.p, (const float *)dRefN.p,
                                                     (ppg_debug_pdf *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_pdf), hipMemcpyDeviceToHost));
    return PPG_OK;
}

// mat_eval / mat_pdf / mat_sample of kernel family `family` and unit `unit` (both checked by the caller), item by item.  A sample outside
// [0, 1] is refused: the plug-ins divide it by a probability and hand it to table lookups (the rough-transmittance slice, a blend's cdf).
static int debugBsdf(ppg_ctx *ctx, const char *who, int family, int unit, uint32_t n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    if (n && (!items || !out)) { ctx->error = std::string(who) + ": no arrays"; return PPG_ERR_INVALID; }
    for (uint32_t i = 0; i < n; ++i) {
        if (items[i].material < 0 || (uint32_t)items[i].material >= ctx->nMaterials) { ctx->error = std::string(who) + ": item " + std::to_string(i) + ": material out of range"; return PPG_ERR_INVALID; }
        const float *u = items[i].sample;
        if (!(u[0] >= 0.0f && u[0] <= 1.0f && u[1] >= 0.0f && u[1] <= 1.0f)) { ctx->error = std::string(who) + ": item " + std::to_string(i) + ": a sample outside [0, 1]"; return PPG_ERR_INVALID; }
    }
    if (n == 0) return PPG_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    if (unit == PPG_DEBUG_BSDF_COMMON) {  // what sort_slice keeps out of the common part of a slice (ppg_kernels.h), k_shade<.., MSET_COMMON> never sees
        std::vector<float4> mats(PPG_MAT_STRIDE * (size_t)ctx->nMaterials);
        HIP_CHECK(hipMemcpy(mats.data(), ctx->scene.materials, mats.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) {
            const float4 *mr = mats.data() + PPG_MAT_STRIDE * (size_t)items[i].material;
            const int type = (int)mr[0].w, flags = ppg_f2u(mr[2].w);
            const uint32_t tex = ppg_f2u(mr[5].x), slots = ppg_f2u(mr[5].y) | ppg_f2u(mr[5].z) | ppg_f2u(mr[5].w);
            const char *why = nullptr;
            if (!(type == PPG_BSDF_DIFFUSE || type == PPG_BSDF_TWOSIDED_DIFFUSE || type == PPG_BSDF_MIRROR || type == PPG_BSDF_CONDUCTOR || type == PPG_BSDF_ROUGHCONDUCTOR ||
                  type == PPG_BSDF_PLASTIC || type == PPG_BSDF_ROUGHPLASTIC)) why = "its BSDF type is not one of the common classes";
            else if (flags & PPG_MAT_MASK) why = "a masked material is not in the common classes";
            else if (slots) why = "a bitmap on specular / alpha / opacity keeps the material out of the common classes";
            else if (tex >> 16) why = "a bump or normal map keeps the material out of the common classes";
            if (why) { ctx->error = std::string(who) + ": item " + std::to_string(i) + ": " + why; return PPG_ERR_INVALID; }
        }
    }
    DebugBuf dItems, dOut;
    HIP_CHECK(dItems.fill(items, (size_t)n * sizeof(ppg_debug_bsdf_item)));
    HIP_CHECK(dOut.fill(nullptr, (size_t)n * sizeof(ppg_debug_bsdf_out)));
    const unsigned int block = 64;
    const int grid = (int)((n + block - 1) / block);
    if (unit == PPG_DEBUG_BSDF_COMMON) ppg_launch_debug_bsdf_common(grid, (int)block, ctx->stream, ctx->scene, n, (const ppg_debug_bsdf_item *)dItems.p, (ppg_debug_bsdf_out *)dOut.p);
    else launcher(ppg_path_kernels[family].debug_bsdf)(unit == PPG_DEBUG_BSDF_LEAN ? 1 : 0, grid, (int)block, ctx->stream, ctx->scene, n, (const ppg_debug_bsdf_item *)dItems.p, (ppg_debug_bsdf_out *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n * sizeof(ppg_debug_bsdf_out), hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_debug_bsdf_as(ppg_ctx *ctx, int32_t family, int32_t unit, uint32_t n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_bsdf_as: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    int fam = 0;
    if (const int rc = debugFamily(ctx, "ppg_debug_bsdf_as", family, &fam)) return rc;
    if (family < 0) unit = ctx->fullMaterials ? PPG_DEBUG_BSDF_FULL : PPG_DEBUG_BSDF_LEAN;
    if (unit != PPG_DEBUG_BSDF_FULL && unit != PPG_DEBUG_BSDF_LEAN && unit != PPG_DEBUG_BSDF_COMMON) { ctx->error = "ppg_debug_bsdf_as: no such unit"; return PPG_ERR_INVALID; }
    if (unit == PPG_DEBUG_BSDF_LEAN && fam != PPG_FAMILY_BASE) { ctx->error = "ppg_debug_bsdf_as: the LEAN functions exist in the base family only"; return PPG_ERR_INVALID; }
    if (unit == PPG_DEBUG_BSDF_COMMON && fam != PPG_FAMILY_BASE) { ctx->error = "ppg_debug_bsdf_as: the COMMON unit exists in the base family only"; return PPG_ERR_INVALID; }
    if (unit == PPG_DEBUG_BSDF_LEAN && ctx->fullMaterials) { ctx->error = "ppg_debug_bsdf_as: the scene needs the FULL kernels"; return PPG_ERR_INVALID; }
    return debugBsdf(ctx, "ppg_debug_bsdf_as", fam, unit, n, items, out);
}
int ppg_debug_bsdf(ppg_ctx *ctx, uint32_t n, const ppg_debug_bsdf_item *items, ppg_debug_bsdf_out *out) {
    if (!ctx->haveScene) { ctx->error = "no scene"; return PPG_ERR_STATE; }
    if (ctx->renderOpen) { ctx->error = "ppg_debug_bsdf: not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    const int family = std::max(sceneFamily(ctx->scene, ctx->mediaArgs, ctx->hetArgs), PPG_FAMILY_EXT);  // (as before the base and shapes families compiled the hook's kernel)
    return debugBsdf(ctx, "ppg_debug_bsdf", family, PPG_DEBUG_BSDF_FULL, n, items, out);
}

// include/ppg_mathcheck.h in one family's TRACE unit, or (family = -1) in this translation unit's host code; no scene is needed
static int debugMathRefusal(ppg_ctx *ctx, const char *who, int32_t family, int32_t via, int32_t op) {
    if (ctx->renderOpen) { ctx->error = std::string(who) + ": not between ppg_begin_render and ppg_end_render"; return PPG_ERR_STATE; }
    if (!ppg_mathcheck_known(op)) { ctx->error = std::string(who) + ": no such op"; return PPG_ERR_INVALID; }
    if (family < -1 || family >= PPG_DEBUG_FAMILIES) { ctx->error = std::string(who) + ": no such kernel family"; return PPG_ERR_INVALID; }
    if (via != 0 && via != 1) { ctx->error = std::string(who) + ": via is 0 (the header's functions) or 1 (the module's dm_ copies)"; return PPG_ERR_INVALID; }
    if (via == 1 && family < 0) { ctx->error = std::string(who) + ": the host has no dm_ copies"; return PPG_ERR_INVALID; }
    if (via == 1 && !ppg_mathcheck_has_dm(op)) { ctx->error = std::string(who) + ": the kernels have no dm_ copy of this op"; return PPG_ERR_INVALID; }
    return PPG_OK;
}
int ppg_debug_math_eval(ppg_ctx *ctx, int32_t family, int32_t via, int32_t op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1) {
    if (const int rc = debugMathRefusal(ctx, "ppg_debug_math_eval", family, via, op)) return rc;
    if (n && (!a || !b || !out0 || !out1)) { ctx->error = "ppg_debug_math_eval: no arrays"; return PPG_ERR_INVALID; }
    if (n == 0) return PPG_OK;
    const bool two = ppg_mathcheck_outputs(op) == 2;
    if (family < 0) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t ua = ppg_mathcheck_arg_a(op, i, a[i]);
            if (!ppg_mathcheck_in_domain(op, ua, b[i])) continue;
            uint32_t o0 = 0u, o1 = 0u;
            ppg_mathcheck_eval(op, ua, b[i], &o0, &o1);
            out0[i] = o0;
            if (two) out1[i] = o1;
        }
        return PPG_OK;
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    DebugBuf dA, dB, d0, d1;
    HIP_CHECK(dA.fill(a, bytes));
    HIP_CHECK(dB.fill(b, bytes));
    HIP_CHECK(d0.fill(out0, bytes));  // (an element outside the op's domain keeps what the caller sent)
    HIP_CHECK(d1.fill(out1, bytes));
    launcher(ppg_path_kernels[family].debug_math_eval)(ctx->stream, via, op, n, (const uint32_t *)dA.p, (const uint32_t *)dB.p, (uint32_t *)d0.p, (uint32_t *)d1.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out0, d0.p, bytes, hipMemcpyDeviceToHost));
    if (two) HIP_CHECK(hipMemcpy(out1, d1.p, bytes, hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_debug_math_checksum(ppg_ctx *ctx, int32_t family, int32_t via, int32_t op, uint32_t first_block, uint32_t n_blocks, uint64_t *out) {
    if (const int rc = debugMathRefusal(ctx, "ppg_debug_math_checksum", family, via, op)) return rc;
    if (!ppg_mathcheck_unary(op)) { ctx->error = "ppg_debug_math_checksum: only the ops of one argument have block checksums"; return PPG_ERR_INVALID; }
    if (first_block > PPG_MATHCHECK_BLOCKS || n_blocks > PPG_MATHCHECK_BLOCKS - first_block) { ctx->error = "ppg_debug_math_checksum: blocks beyond 256"; return PPG_ERR_INVALID; }
    if (n_blocks && !out) { ctx->error = "ppg_debug_math_checksum: no array"; return PPG_ERR_INVALID; }
    if (n_blocks == 0) return PPG_OK;
    if (family < 0) {
        std::vector<std::thread> pool;  // one thread per block, sixteen at a time
        for (uint32_t k0 = 0; k0 < n_blocks; k0 += 16) {
            for (uint32_t k = k0; k < std::min(n_blocks, k0 + 16); ++k)
                pool.emplace_back([=] {
                    const uint32_t base = (first_block + k) << PPG_MATHCHECK_BLOCK_BITS;
                    uint64_t sum = 0;
                    for (uint32_t i = 0; i < (1u << PPG_MATHCHECK_BLOCK_BITS); ++i) sum += ppg_mathcheck_term(op, base | i);
                    out[k] = sum;
                });
            for (auto &t : pool) t.join();
            pool.clear();
        }
        return PPG_OK;
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    ctx->quiesce();
    DebugBuf dOut;
    HIP_CHECK(dOut.fill(nullptr, (size_t)n_blocks * sizeof(uint64_t)));
    HIP_CHECK(hipMemsetAsync(dOut.p, 0, (size_t)n_blocks * sizeof(uint64_t), ctx->stream));
    launcher(ppg_path_kernels[family].debug_math_checksum)(ctx->stream, via, op, first_block, n_blocks, (unsigned long long *)dOut.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n_blocks * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PPG_OK;
}

int ppg_debug_rfilter_table(const ppg_rfilter *f, float table[32], float *radius, int32_t *border) {
    if (!f || !table || !radius || !border) return PPG_ERR_INVALID;
    std::string err;
    return rfilterTable(f, table, radius, border, err);
}

int ppg_release_cached_memory(int32_t device) {
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess) return PPG_ERR_DEVICE;
    g_blockCache.trim();
    (void)hipSetDevice(prev);
    return PPG_OK;
}

int ppg_render(ppg_ctx *ctx) {  // GP:1516-1585
    NEED_SCENE
    int rc = beginRender(ctx);
    if (rc) return rc;
    rc = ctx->budgetType == 0 ? renderSPP(ctx) : renderTime(ctx);
    if (rc) { ctx->renderOpen = false; return rc; }
    return endRender(ctx);
}

int ppg_read_film(ppg_ctx *ctx, float *rgb) {
    NEED_SCENE
    const int n = ctx->W * ctx->H;
    if (!ctx->d_film.p || !ctx->d_tmp.p) { ctx->error = "nothing rendered"; return PPG_ERR_STATE; }
    hipLaunchKernelGGL(k_normalise, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, ctx->d_film.p, ctx->d_filmW.p, ctx->d_tmp.p);
    HIP_CHECK(hipMemcpyAsync(rgb, ctx->d_tmp.p, 3 * (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PPG_OK;
}
int ppg_read_variance(ppg_ctx *ctx, float *rgb) {
    NEED_SCENE
    if (!ctx->d_var.p) { ctx->error = "nothing rendered"; return PPG_ERR_STATE; }
    HIP_CHECK(hipMemcpy(rgb, ctx->d_var.p, 3 * (size_t)ctx->W * ctx->H * 4, hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_dump_sdtree(ppg_ctx *ctx, const char *path) { NEED_TREE return dumpSDTreeFile(ctx, path); }

int ppg_load_sdtree(ppg_ctx *ctx, const char *path, const ppg_sdtree_load *opts) {
    if (!ctx) return PPG_ERR_INVALID;
    if (!ctx->treeAlive || !ctx->renderOpen) { ctx->error = "ppg_load_sdtree: render not begun (call it after ppg_begin_render)"; return PPG_ERR_STATE; }
    if (ctx->iterOpen) { ctx->error = "ppg_load_sdtree: an iteration is open (call it before ppg_begin_iteration, or after ppg_build_sdtree)"; return PPG_ERR_STATE; }
    if (ctx->shardWorld > 1) { ctx->error = "ppg_load_sdtree: a sharded render (ppg_set_shard with world > 1) is not supported yet"; return PPG_ERR_INVALID; }
    if (!path) { ctx->error = "ppg_load_sdtree: no path"; return PPG_ERR_INVALID; }
    ppg_sdtree_load o{};
    if (opts) o = *opts;
    if (o.iter < 0 || o.iter > 30 || o.passes_rendered < 0 || o._reserved[0] || o._reserved[1]) {
        ctx->error = "ppg_load_sdtree: iter must be 0 .. 30, passes_rendered >= 0 and the reserved fields 0";
        return PPG_ERR_INVALID;
    }
    NEED_TREE
    return loadSDTreeFile(ctx, path, o.iter, o.passes_rendered);
}

int ppg_sdtree_info_get(ppg_ctx *ctx, ppg_sdtree_info *info) {
    NEED_TREE
    memset(info, 0, sizeof *info);
    info->n_stree_nodes = (uint32_t)ctx->snodes.size();
    std::vector<LeafHdr> dh(ctx->hdr);
    if (ctx->d_hdr.p && ctx->d_hdr.cap >= dh.size()) HIP_CHECK(hipMemcpy(dh.data(), ctx->d_hdr.p, dh.size() * sizeof(LeafHdr), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ctx->snodes.size(); ++i)
        if (ctx->snodes[i].isLeaf()) { info->n_leaves++; info->n_sampling_nodes += ctx->hdr[i].s_num; info->n_building_nodes += dh[i].b_num; }
    for (int a = 0; a < 3; ++a) { info->aabb_min[a] = ctx->treeMin[a]; info->aabb_max[a] = ctx->treeMax[a]; }
    info->iter = ctx->iter; info->is_built = ctx->isBuilt;
    return PPG_OK;
}

int ppg_sdtree_read_stree(ppg_ctx *ctx, int32_t *axis, uint32_t *children) {
    NEED_TREE
    for (size_t i = 0; i < ctx->snodes.size(); ++i) { axis[i] = ctx->snodes[i].axis; children[2 * i] = ctx->snodes[i].child[0]; children[2 * i + 1] = ctx->snodes[i].child[1]; }
    return PPG_OK;
}

int ppg_sdtree_read_dtree_headers(ppg_ctx *ctx, int32_t which, uint64_t *offset, uint32_t *num_nodes, int32_t *max_depth, float *sum, double *stat_weight) {
    NEED_TREE
    std::vector<LeafHdr> dh(ctx->hdr.size());
    std::vector<unsigned long long> bw(ctx->hdr.size(), 0);
    { int rc = foldWeights(ctx); if (rc) return rc; }
    if (ctx->d_hdr.p) {
        HIP_CHECK(hipMemcpy(dh.data(), ctx->d_hdr.p, dh.size() * sizeof(LeafHdr), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(bw.data(), ctx->d_bweight.p, bw.size() * 8, hipMemcpyDeviceToHost));
    } else dh = ctx->hdr;
    uint64_t off = 0;
    for (size_t i = 0; i < ctx->snodes.size(); ++i) {
        if (!ctx->snodes[i].isLeaf()) { offset[i] = 0; num_nodes[i] = 0; max_depth[i] = 0; sum[i] = 0; stat_weight[i] = 0; continue; }
        const LeafHdr &h = dh[i];
        offset[i] = off;
        if (which == 0) { num_nodes[i] = h.s_num; max_depth[i] = h.s_depth; sum[i] = h.s_sum; stat_weight[i] = h.s_statw; off += h.s_num; }
        else {
            num_nodes[i] = h.b_num; max_depth[i] = h.b_depth; sum[i] = 0.0f;
            stat_weight[i] = (double)bw[i] / 16777216.0;  // the accumulator of the current iteration
            off += h.b_num;
        }
    }
    return PPG_OK;
}

int ppg_sdtree_read_dtree_nodes(ppg_ctx *ctx, int32_t which, float *sums, uint16_t *children, uint64_t *fixed_sums) {
    NEED_TREE
    std::vector<float> s; std::vector<uint16_t> c; std::vector<uint64_t> f;
    int rc = gatherDTrees(ctx, which, s, c, fixed_sums ? &f : nullptr);
    if (rc) return rc;
    memcpy(sums, s.data(), s.size() * 4);
    memcpy(children, c.data(), c.size() * 2);
    if (fixed_sums) memcpy(fixed_sums, f.data(), f.size() * 8);
    return PPG_OK;
}

int ppg_sdtree_read_adam(ppg_ctx *ctx, float *theta) {
    NEED_TREE
    std::vector<LeafHdr> dh(ctx->hdr.size());
    if (ctx->d_hdr.p) HIP_CHECK(hipMemcpy(dh.data(), ctx->d_hdr.p, dh.size() * sizeof(LeafHdr), hipMemcpyDeviceToHost));
    else dh = ctx->hdr;
    for (size_t i = 0; i < dh.size(); ++i) theta[i] = dh[i].theta;
    return PPG_OK;
}

int ppg_sdtree_stat_buffers(ppg_ctx *ctx, void **dev_sums, uint64_t *n_sums, void **dev_weights, uint64_t *n_weights) {
    NEED_TREE
    { int rc = foldWeights(ctx); if (rc) return rc; }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *dev_sums = ctx->d_bacc.p; *n_sums = ctx->nBuildingNodes * 4;
    *dev_weights = ctx->d_bweight.p; *n_weights = ctx->snodes.size();
    return PPG_OK;
}
int ppg_film_buffers(ppg_ctx *ctx, void **dev_rgb_sum, void **dev_weight) {
    NEED_TREE
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *dev_rgb_sum = ctx->d_film.p; *dev_weight = ctx->d_filmW.p;
    return PPG_OK;
}
int ppg_image_buffers(ppg_ctx *ctx, void **dev_image, void **dev_sq_image, void **dev_weight) {
    NEED_TREE
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *dev_image = ctx->d_image.p; *dev_sq_image = ctx->d_sq.p; *dev_weight = ctx->d_imageW.p;
    return PPG_OK;
}

int ppg_set_stop_hook(ppg_ctx *ctx, ppg_stop_hook hook, void *user) { ctx->stopHook = hook; ctx->stopHookUser = user; return PPG_OK; }
int ppg_exchange_stream(ppg_ctx *ctx, void **hip_stream) { *hip_stream = (void *)ctx->stream; return PPG_OK; }
int32_t ppg_final_group_passes(int32_t n_passes) {
    const int32_t n = std::max(1, n_passes);
    return 16 * ((n + 1023) / 1024);
}
int ppg_final_partials(ppg_ctx *ctx, void **dev, uint64_t *n_floats) {
    NEED_TREE
    *dev = nullptr; *n_floats = 0;
    if (!ctx->partialsPending) return PPG_OK;  // not a sharded final iteration: image / squared image / weights are exchanged as usual
    const size_t n = ctx->nPixAll;
    if (!ctx->partialsExported) {  // the film of this iteration so far (tile-sharded training passes of an `automatic` render) travels in the head
        HIP_CHECK(hipMemcpyAsync(ctx->d_partials.p, ctx->d_film.p, 3 * n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(ctx->d_partials.p + 3 * n, ctx->d_filmW.p, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->partialsExported = true;
    }
    *dev = ctx->d_partials.p; *n_floats = 4 * n + (uint64_t)ctx->pendingGroups * 7 * n;
    return PPG_OK;
}
int ppg_final_partials_commit(ppg_ctx *ctx) {
    NEED_TREE
    if (!ctx->partialsPending || !ctx->partialsExported) { ctx->error = "ppg_final_partials_commit: nothing to commit"; return PPG_ERR_STATE; }
    const size_t n = ctx->nPixAll;
    HIP_CHECK(hipMemcpyAsync(ctx->d_film.p, ctx->d_partials.p, 3 * n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(ctx->d_filmW.p, ctx->d_partials.p + 3 * n, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    addGroups(ctx, 0, ctx->pendingGroups);
    HIP_CHECK(hipGetLastError());
    ctx->partialsPending = false; ctx->partialsExported = false;
    return PPG_OK;
}
int ppg_set_pass_hook(ppg_ctx *ctx, ppg_pass_hook hook, void *user) { ctx->passHook = hook; ctx->passHookUser = user; return PPG_OK; }
int ppg_set_footprint_hook(ppg_ctx *ctx, ppg_footprint_hook hook, void *user) {
    if (!hook && ctx->exchangesFootprints()) {
        ctx->error = "ppg_set_footprint_hook: a sharded filtered render is set up on this context — it cannot do without the hook";
        return PPG_ERR_INVALID;
    }
    ctx->footHook = hook; ctx->footHookUser = user;
    return PPG_OK;
}
uint64_t ppg_footprint_halo_floats(int32_t width, int32_t height, int32_t tile_size, int32_t world, int32_t border) {
    if (width < 1 || height < 1 || tile_size < 1 || world <= 1 || border < 1) return 0;
    uint64_t m = 0;
    forEachBorderSlot(width, height, tile_size, world, border, [&](unsigned int, unsigned int, int, int) { ++m; });
    return 7 * m;
}
int ppg_adam_records(ppg_ctx *ctx, void **dev_records, uint64_t *n) {
    NEED_TREE
    if (!ctx->inHook) { ctx->error = "ppg_adam_records: only valid inside the round hook"; return PPG_ERR_STATE; }
    *dev_records = ctx->hookReplaced ? (void *)ctx->d_adamRecs.p : (void *)ctx->d_adamRecsOut.p;
    *n = ctx->hookCount;
    return PPG_OK;
}
int ppg_hook_phase(ppg_ctx *ctx, int32_t *phase) {
    if (!ctx || !phase) return PPG_ERR_INVALID;
    *phase = ctx->hookPhase;
    return PPG_OK;
}
int ppg_adam_records_by_owner(ppg_ctx *ctx, int32_t world, void **dev_records, uint64_t *counts) {
    if (!ctx || !dev_records || !counts || world < 1) return PPG_ERR_INVALID;
    if (!ctx->inHook || ctx->hookPhase != 0) { ctx->error = "ppg_adam_records_by_owner: only valid in phase 0 of the round hook"; return PPG_ERR_STATE; }
    HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned int nNodes = (unsigned int)ctx->snodes.size();
    const unsigned int seg = (nNodes + (unsigned int)world - 1u) / (unsigned int)world;
    const unsigned int n = (unsigned int)ctx->hookCount;  // the valid records, in key order: d_adamKeys[1] / d_adamRecsOut
    HIP_CHECK(ctx->d_ownerBounds.reserve((size_t)world + 1));
    std::vector<unsigned long long> b((size_t)world + 1, 0ull);
    if (n) {
        hipLaunchKernelGGL(k_owner_bounds, dim3(((unsigned int)world + 1u + 63u) / 64u), dim3(64), 0, ctx->stream, ctx->d_adamKeys[1].p, n, seg, (unsigned int)world, ctx->d_ownerBounds.p);
        HIP_CHECK(hipMemcpyAsync(b.data(), ctx->d_ownerBounds.p, b.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    for (int32_t r = 0; r < world; ++r) counts[r] = b[(size_t)r + 1] - b[(size_t)r];
    *dev_records = ctx->d_adamRecsOut.p;
    ctx->ownerMode = true;
    return PPG_OK;
}
int ppg_adam_state(ppg_ctx *ctx, int32_t world, void **dev_state, uint64_t *segment) {
    if (!ctx || !dev_state || !segment || world < 1) return PPG_ERR_INVALID;
    if (!ctx->inHook || ctx->hookPhase != 1) { ctx->error = "ppg_adam_state: only valid in phase 1 of the round hook"; return PPG_ERR_STATE; }
    HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned int nNodes = (unsigned int)ctx->snodes.size();
    const size_t seg = ((size_t)nNodes + (size_t)world - 1) / (size_t)world;
    const size_t words = (size_t)world * seg * 6;
    HIP_CHECK(ctx->d_adamState.reserve(std::max<size_t>(words, 6)));
    HIP_CHECK(hipMemsetAsync(ctx->d_adamState.p, 0, words * 4, ctx->stream));
    hipLaunchKernelGGL((k_adam_state<false>), dim3((nNodes + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_hdr.p, nNodes, ctx->d_adamState.p);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *dev_state = ctx->d_adamState.p; *segment = seg;
    return PPG_OK;
}
int ppg_adam_state_commit(ppg_ctx *ctx) {
    if (!ctx) return PPG_ERR_INVALID;
    if (!ctx->inHook || ctx->hookPhase != 1 || !ctx->d_adamState.p) { ctx->error = "ppg_adam_state_commit: call ppg_adam_state first"; return PPG_ERR_STATE; }
    HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned int nNodes = (unsigned int)ctx->snodes.size();
    hipLaunchKernelGGL((k_adam_state<true>), dim3((nNodes + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_hdr.p, nNodes, ctx->d_adamState.p);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PPG_OK;
}
int ppg_adam_records_replace(ppg_ctx *ctx, const void *dev_records, uint64_t n) {
    NEED_TREE
    if (!ctx->inHook) { ctx->error = "ppg_adam_records_replace: only valid inside the round hook"; return PPG_ERR_STATE; }
    if (n > 0xfffffff0ull) { ctx->error = "too many Adam records in one round"; return PPG_ERR_NOMEM; }
    if (n && dev_records == (const void *)ctx->d_adamRecs.p) { ctx->error = "ppg_adam_records_replace: source aliases the destination"; return PPG_ERR_INVALID; }
    HIP_CHECK(ctx->d_adamRecs.reserve(std::max<size_t>(1, (size_t)n)));
    if (n) HIP_CHECK(hipMemcpyAsync(ctx->d_adamRecs.p, dev_records, (size_t)n * sizeof(AdamRec), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->hookReplaced = true; ctx->hookCount = n;
    return PPG_OK;
}

int ppg_query_pdf(ppg_ctx *ctx, uint32_t n, const float *positions, const float *dirs, float *pdf_out) {
    NEED_TREE
    if (n == 0) return PPG_OK;
    DevBuf<float> dp, dd, dout;
    HIP_CHECK(dp.reserve(3 * (size_t)n)); HIP_CHECK(dd.reserve(3 * (size_t)n)); HIP_CHECK(dout.reserve(n));
    HIP_CHECK(hipMemcpy(dp.p, positions, 12 * (size_t)n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dd.p, dirs, 12 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_query_pdf, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->devTree(), n, dp.p, dd.p, dout.p);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(pdf_out, dout.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return PPG_OK;
}
int ppg_query_sample(ppg_ctx *ctx, uint32_t n, const float *positions, uint64_t seed, float *dirs_out) {
    NEED_TREE
    if (n == 0) return PPG_OK;
    DevBuf<float> dp, dout;
    HIP_CHECK(dp.reserve(3 * (size_t)n)); HIP_CHECK(dout.reserve(3 * (size_t)n));
    HIP_CHECK(hipMemcpy(dp.p, positions, 12 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_query_sample, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->devTree(), n, dp.p, (unsigned long long)seed, dout.p);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    HIP_CHECK(hipMemcpy(dirs_out, dout.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
    return PPG_OK;
}

int ppg_debug_stree_depth(const uint32_t *children, uint32_t n_nodes, int32_t spatial_filter, uint32_t *depth) {  // include/ppg_testhooks.h
    if (!children || !depth || n_nodes == 0) return PPG_ERR_INVALID;
    return streeDepthCheck(children, n_nodes, spatial_filter, depth);
}

// ---- ppg_debug_commit (include/ppg_testhooks.h): explicit vertices through the commit and the round end of a batch ----
// the host-side checks of ppg_debug_commit: nullptr when the arrays may be read and the counts hold, else the complaint
static const char *debugCommitCheck(const ppg_debug_commit_in *in, int32_t max_vertices, int32_t round, int32_t positions_known, uint32_t flag_shift) {
    if (!in) return "ppg_debug_commit: in is NULL";
    if (in->route < PPG_DEBUG_COMMIT || in->route > PPG_DEBUG_COMMIT_RECORDS_SPLIT) return "ppg_debug_commit: route: no such route";
    if (in->n_paths >= PPG_ADAM_DEFER_PATH_BIT) return "ppg_debug_commit: n_paths must be below 2^26";
    if (max_vertices < 1 || max_vertices > PPG_MAX_VERTICES) return "ppg_debug_commit: the context has no vertex slots";
    if (in->n_paths && (!in->nv || !in->key || !in->dim)) return "ppg_debug_commit: nv, key and dim are needed per path";
    uint64_t sum = 0;
    for (uint32_t i = 0; i < in->n_paths; ++i) {
        if (in->nv[i] > (uint32_t)max_vertices) return "ppg_debug_commit: nv: a path has more vertices than the context's max_vertices";
        sum += in->nv[i];
    }
    if (sum != in->n_vertices) return "ppg_debug_commit: n_vertices is not the sum of nv";
    if (sum && (!in->p || !in->d || !in->radiance || !in->throughput || !in->bsdf_val || !in->wo_pdf || !in->bsdf_pdf || !in->dtree_pdf || !in->is_delta))
        return "ppg_debug_commit: a per-vertex array is NULL";
    if (in->route >= PPG_DEBUG_COMMIT_RECORDS) {
        if (!round) return "ppg_debug_commit: route: the record routes need a round of the optimiser (a bsdfSamplingFractionLoss and a built tree)";
        if (!positions_known) return "ppg_debug_commit: route: the record routes need known record positions (no box spatial filter, no kickstart luminaire sampling)";
        if (flag_shift >= 63u) return "ppg_debug_commit: route: the S-tree leaves no key bit for the record routes";
    }
    return nullptr;
}

int ppg_debug_commit(ppg_ctx *ctx, const ppg_debug_commit_in *in, ppg_debug_commit_out *out) {
    if (!ctx) return PPG_ERR_INVALID;
    NEED_TREE
    if (!ctx->iterOpen || ctx->inHook) { ctx->error = "ppg_debug_commit: only between ppg_begin_iteration(ctx, 0) and ppg_build_sdtree, outside the round hook"; return PPG_ERR_STATE; }
    if (ctx->passHook) { ctx->error = "ppg_debug_commit: not while a round hook is installed (ppg_set_pass_hook): it may replace the round's records"; return PPG_ERR_STATE; }
    if (!out) { ctx->error = "ppg_debug_commit: out is NULL"; return PPG_ERR_INVALID; }
    const bool round = ctx->loss != LOSS_NONE && ctx->isBuilt;
    const bool known = recordPositionsKnown(ctx->spatialFilter, ctx->doNee, ctx->nee);
    const unsigned int flagShift = adamFlagShift(ctx->snodes.size());
    if (const char *why = debugCommitCheck(in, ctx->maxVertices, round ? 1 : 0, known ? 1 : 0, flagShift)) { ctx->error = why; return PPG_ERR_INVALID; }
    if ((out->keys_cap && !out->keys) || (out->records_cap && !out->records)) { ctx->error = "ppg_debug_commit: out: a capacity without its array"; return PPG_ERR_INVALID; }
    if (round && ctx->snodes.size() >= (1u << 24)) { ctx->error = "S-tree exceeds 2^24 nodes with a bsdfSamplingFractionLoss"; return PPG_ERR_NOMEM; }
    ctx->quiesce();
    hipStream_t s = ctx->stream;
    const unsigned int n = in->n_paths, nNodes = (unsigned int)ctx->snodes.size();
    const bool records = in->route >= PPG_DEBUG_COMMIT_RECORDS;
    const bool split = in->route == PPG_DEBUG_COMMIT_SPLIT || in->route == PPG_DEBUG_COMMIT_RECORDS_SPLIT;
    out->committed = 0; out->n_keys = 0; out->n_records = 0;
    size_t nRecords = 0;
    if (n) {
        // the arrays, and the paths of a batch over them (one array per field, as allocPaths lays them out)
        unsigned int slots = 1;
        std::vector<unsigned int> first(n), lateList;
        std::vector<unsigned char> lateFlag(n, 0);
        {
            uint64_t f = 0;
            for (unsigned int i = 0; i < n; ++i) {
                first[i] = (unsigned int)f; f += in->nv[i]; slots = std::max(slots, in->nv[i]);
                if (split && in->late && in->late[i]) { lateFlag[i] = 1; lateList.push_back(i); }
            }
            if (f > 0xfffffff0ull) { ctx->error = "ppg_debug_commit: n_vertices: too many vertices"; return PPG_ERR_INVALID; }
        }
        const size_t nvx = (size_t)in->n_vertices, nv4 = (size_t)slots * n * sizeof(float4);
        const bool filtered = ctx->spatialFilter != SF_NEAREST;
        DebugBuf aNv, aKey, aDim, aFirst, aP, aD, aRad, aThr, aBsdf, aWo, aBp, aDp, aDelta, bMisc, bVd, bVthr, bVbsdf, bVrad, bVo, bVvox, bPix, bStats, bLate, bList, bListN;
        HIP_CHECK(aNv.fill(in->nv, (size_t)n * 4)); HIP_CHECK(aKey.fill(in->key, (size_t)n * 4)); HIP_CHECK(aDim.fill(in->dim, (size_t)n * 4));
        HIP_CHECK(aFirst.fill(first.data(), (size_t)n * 4));
        HIP_CHECK(aP.fill(in->p, nvx * 12)); HIP_CHECK(aD.fill(in->d, nvx * 12)); HIP_CHECK(aRad.fill(in->radiance, nvx * 12));
        HIP_CHECK(aThr.fill(in->throughput, nvx * 12)); HIP_CHECK(aBsdf.fill(in->bsdf_val, nvx * 12));
        HIP_CHECK(aWo.fill(in->wo_pdf, nvx * 4)); HIP_CHECK(aBp.fill(in->bsdf_pdf, nvx * 4)); HIP_CHECK(aDp.fill(in->dtree_pdf, nvx * 4));
        HIP_CHECK(aDelta.fill(in->is_delta, nvx));
        HIP_CHECK(bMisc.fill(nullptr, (size_t)n * sizeof(uint4)));
        HIP_CHECK(bVd.fill(nullptr, nv4)); HIP_CHECK(bVthr.fill(nullptr, nv4)); HIP_CHECK(bVbsdf.fill(nullptr, nv4)); HIP_CHECK(bVrad.fill(nullptr, nv4));
        if (filtered) { HIP_CHECK(bVo.fill(nullptr, nv4)); HIP_CHECK(bVvox.fill(nullptr, nv4)); }
        HIP_CHECK(bPix.fill(nullptr, (size_t)n * 4));
        const int grid = wavefrontGrid(ctx->nBlocks, ctx->tuneBlocksSmall, ctx->tuneSmallPaths, n, ctx->queues.cap);
        HIP_CHECK(bStats.fill(nullptr, (size_t)grid * sizeof(BlockStats)));
        HIP_CHECK(hipMemsetAsync(bStats.p, 0, (size_t)grid * sizeof(BlockStats), s));
        HIP_CHECK(bLate.fill(lateFlag.data(), n));
        const unsigned long long listN = lateList.size();
        HIP_CHECK(bList.fill(lateList.data(), lateList.size() * 4)); HIP_CHECK(bListN.fill(&listN, 8));
        hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, s, (unsigned int *)bPix.p, n);
        PathState P{};
        P.n_paths = n; P.n_pix = n; P.pixels = (const unsigned int *)bPix.p;
        P.misc = {(uint4 *)bMisc.p, 1u};
        P.v_d = {(float4 *)bVd.p, 1u}; P.v_thr = {(float4 *)bVthr.p, 1u}; P.v_bsdf = {(float4 *)bVbsdf.p, 1u}; P.v_rad = {(float4 *)bVrad.p, 1u};
        P.v_o = {filtered ? (float4 *)bVo.p : nullptr, 1u}; P.v_vox = {filtered ? (float4 *)bVvox.p : nullptr, 1u};
        const DebugCommitArrays A{(const unsigned int *)aNv.p, (const unsigned int *)aKey.p, (const unsigned int *)aDim.p, (const unsigned int *)aFirst.p,
                                  (const float *)aP.p, (const float *)aD.p, (const float *)aRad.p, (const float *)aThr.p, (const float *)aBsdf.p,
                                  (const float *)aWo.p, (const float *)aBp.p, (const float *)aDp.p, (const unsigned char *)aDelta.p};
        hipLaunchKernelGGL(k_debug_commit_fill, dim3((n + 255) / 256), dim3(256), 0, s, P, ctx->devTree(), A, slots);
        HIP_CHECK(hipGetLastError());
        // the round's state, as prepareBatch sets it
        ctx->adamActive = round; ctx->adamFast = round && known; ctx->sortedCommit = records; ctx->adamFlagShift = flagShift;
        struct RoundEnd { ppg_ctx *c; ~RoundEnd() { c->adamActive = false; } } roundEnd{ctx};
        const unsigned char *late = split ? (const unsigned char *)bLate.p : nullptr;
        if (round && !ctx->adamFast) {  // positions handed out as the records are made (prepareBatch)
            const size_t cap = std::max<size_t>((size_t)1 << 16, std::min<size_t>((size_t)48 * n, 0xfffffff0u));
            HIP_CHECK(ctx->d_adamKeys[0].reserve(cap)); HIP_CHECK(ctx->d_adamRecs.reserve(cap));
            HIP_CHECK(hipMemsetAsync(ctx->d_adamCount.p, 0, 8, s));
        }
        if (ctx->adamFast) {  // positions = exclusive scan of the vertex counts; a late path reserves max_vertices (finishPaths)
            HIP_CHECK(ctx->d_adamNv.reserve(n)); HIP_CHECK(ctx->d_adamBase.reserve(n));
            hipLaunchKernelGGL(k_path_nv, dim3((n + 255) / 256), dim3(256), 0, s, P, ctx->d_adamNv.p, late, (unsigned int)ctx->maxVertices);
            size_t bytes = 0;
            HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, ctx->d_adamNv.p, ctx->d_adamBase.p, 0u, (size_t)n, rocprim::plus<unsigned int>(), s));
            HIP_CHECK(ctx->d_sortTemp.reserve(std::max<size_t>(bytes, 16)));
            HIP_CHECK(rocprim::exclusive_scan((void *)ctx->d_sortTemp.p, bytes, ctx->d_adamNv.p, ctx->d_adamBase.p, 0u, (size_t)n, rocprim::plus<unsigned int>(), s));
            unsigned int sumBase = 0, lastNv = 0;
            HIP_CHECK(hipMemcpyAsync(&sumBase, ctx->d_adamBase.p + (n - 1), 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(&lastNv, ctx->d_adamNv.p + (n - 1), 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            nRecords = (size_t)sumBase + lastNv;
            int rc = reserveRoundRecords(ctx, nRecords);
            if (rc) return rc;
        }
        HIP_CHECK(ctx->d_nv8.reserve(n));
        hipLaunchKernelGGL(k_commit_prepare, dim3((n + 255) / 256), dim3(256), 0, s, P, (uint4 *)nullptr, ctx->d_nv8.p, late);
        Queues Q = ctx->queues;
        Q.stats = (BlockStats *)bStats.p; Q.n_blocks = (unsigned int)grid;
        RenderParams R = ctx->params();
        R.img_pixels = n;
        {
            CommitLaunch a{grid, s, P, ctx->devTree(), R, Q, ctx->d_nv8.p, nullptr, nullptr, ctx->d_splat.p, ctx->adamFlagShift};
            timedLaunch(ctx, commitName(records), n, [&] { launchCommitKernels(ctx, a, records); });
        }
        if (split) {  // launchCommit(.., CommitSet::List)
            hipLaunchKernelGGL(k_commit_prepare_list, dim3(std::max(1, std::min(grid, 1024))), dim3(256), 0, s, P, (const unsigned int *)bList.p, (const unsigned long long *)bListN.p, ctx->d_nv8.p);
            CommitLaunch a{grid, s, P, ctx->devTree(), R, Q, ctx->d_nv8.p, (const unsigned int *)bList.p, (const unsigned long long *)bListN.p, ctx->d_splat.p, ctx->adamFlagShift};
            timedLaunch(ctx, commitName(records), 0, [&] { launchCommitKernels(ctx, a, records); });
        }
        HIP_CHECK(hipGetLastError());
        if (round) {  // optimiserRound
            if (!ctx->adamFast) {
                unsigned int cnt[2] = {0, 0};
                HIP_CHECK(hipMemcpyAsync(cnt, ctx->d_adamCount.p, 8, hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                if (cnt[1]) { ctx->error = "Adam record buffer overflow (box spatial filter / next-event estimation with a bsdfSamplingFractionLoss)"; return PPG_ERR_NOMEM; }
                nRecords = cnt[0];
            }
            int rc = applyAdamRound(ctx, nRecords);
            if (rc) return rc;
        }
        { int rc = foldWeights(ctx); if (rc) return rc; }  // (joins the side streams of the round end)
        HIP_CHECK(hipStreamSynchronize(s));
        std::vector<BlockStats> bs((size_t)grid);
        HIP_CHECK(hipMemcpy(bs.data(), bStats.p, bs.size() * sizeof(BlockStats), hipMemcpyDeviceToHost));
        for (const BlockStats &b : bs) out->committed += b.committed;
        if (round && nRecords) {  // the sorted keys without the holes; the optimiser's records are those without the flag bit
            std::vector<unsigned long long> keys(nRecords);
            std::vector<unsigned int> idx(nRecords);
            std::vector<AdamRec> recs(nRecords);
            static_assert(sizeof(AdamRec) == sizeof(ppg_adam_record), "AdamRec = ppg_adam_record");
            HIP_CHECK(hipMemcpy(keys.data(), ctx->d_adamKeys[1].p, nRecords * 8, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(idx.data(), ctx->d_adamIdx[1].p, nRecords * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(recs.data(), ctx->d_adamRecs.p, nRecords * sizeof(AdamRec), hipMemcpyDeviceToHost));
            const unsigned long long flag = records ? (1ull << flagShift) : ~0ull;
            for (size_t k = 0; k < nRecords; ++k) {
                if (keys[k] == ~0ull) continue;
                if (out->n_keys < out->keys_cap) out->keys[out->n_keys] = keys[k];
                ++out->n_keys;
                if (keys[k] >= flag) continue;
                if (idx[k] >= nRecords) { ctx->error = "internal: a record index beyond the round's positions"; return PPG_ERR_STATE; }
                if (out->n_records < out->records_cap) memcpy(&out->records[out->n_records], &recs[idx[k]], sizeof(AdamRec));
                ++out->n_records;
            }
        }
    }
    if (out->adam_state) {
        DebugBuf st;
        HIP_CHECK(st.fill(nullptr, (size_t)nNodes * 24));
        hipLaunchKernelGGL((k_adam_state<false>), dim3((nNodes + 255u) / 256u), dim3(256), 0, s, ctx->d_hdr.p, nNodes, (unsigned int *)st.p);
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipMemcpy(out->adam_state, st.p, (size_t)nNodes * 24, hipMemcpyDeviceToHost));
    }
    return PPG_OK;
}

int ppg_set_adam_regions(ppg_ctx *ctx, int32_t regions) {  // include/ppg.h "Rounds by image region"
    if (!ctx || regions < 0 || regions > 4096) { if (ctx) ctx->error = "ppg_set_adam_regions: 0 .. 4096"; return PPG_ERR_INVALID; }
    ctx->adamRegions = regions >= 2 ? regions : 0;
    return PPG_OK;
}

int ppg_debug_set_defer_depth(ppg_ctx *ctx, int32_t depth) {  // include/ppg_testhooks.h
    if (!ctx || depth < 1 || depth > 64) return PPG_ERR_INVALID;
    ctx->deferDepthAdam = depth;
    return PPG_OK;
}

int ppg_enable_kernel_timing(ppg_ctx *ctx, int32_t enable) {
    ctx->timer.reset();
    ctx->bvhNodesVisited = ctx->bvhTrisTested = 0; ctx->tailLongestSum = 0; ctx->shadeCommonRays = 0;
    ctx->timer.enabled = enable != 0;
    return PPG_OK;
}
int ppg_kernel_times(ppg_ctx *ctx, ppg_kernel_time *out, uint32_t cap, uint32_t *n) {
    ctx->timer.resolve();
    uint32_t k = 0;
    for (size_t i = 0; i < ctx->timer.names.size() && k < cap; ++i, ++k) {
        out[k].name = ctx->timer.names[i].c_str(); out[k].ms = ctx->timer.ms[i]; out[k].launches = ctx->timer.launches[i]; out[k].units = ctx->timer.units[i];
        // the two launches over a sorted slice were both booked with the slice's rays: the common classes' share was counted by sort_slice
        if (ctx->timer.names[i] == "k_shade<common>") out[k].units = ctx->shadeCommonRays;
        else if (ctx->timer.names[i] == "k_shade<rest>") out[k].units = ctx->timer.units[i] > ctx->shadeCommonRays ? ctx->timer.units[i] - ctx->shadeCommonRays : 0;
    }
    // two pseudo entries for the roofline of k_trace on BVH scenes: `units` = BVH4 nodes visited / triangles tested by its launches
    if (k + 2 <= cap && ctx->bvhNodesVisited) {
        out[k].name = "bvh_nodes_visited"; out[k].ms = 0; out[k].launches = 0; out[k].units = ctx->bvhNodesVisited; ++k;
        out[k].name = "bvh_triangles_tested"; out[k].ms = 0; out[k].launches = 0; out[k].units = ctx->bvhTrisTested; ++k;
    }
    // ... and one for k_tail: `units` = sum over its launches of the longest path (bounces) each finished — a launch of k_tail cannot be
    // shorter than its longest path's chain of dependent bounces
    if (k + 1 <= cap && ctx->tailLongestSum) { out[k].name = "tail_longest_paths_sum"; out[k].ms = 0; out[k].launches = 0; out[k].units = ctx->tailLongestSum; ++k; }
    *n = k;
    return PPG_OK;
}

}  // extern "C"
