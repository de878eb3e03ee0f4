// ppg_batch_plan.h — what renderBatch (ppg_hip.hip) DECIDES about a batch, apart from what it launches: plain values in, plain values out, no
// device, no context.  Almost all of it is scheduling only — integer accumulation and the fixed film order make a render bit-equal under
// every schedule —, so no picture can show a mistake here: tests/batch_plan_check.cpp checks these functions on the host, case by case.
// The table of the shapes a batch can take is in DESIGN.md ("Launch structure on MI355X").
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ppg_plan {

// values of ppg_kernels.h and include/ppg.h this header needs (ppg_hip.hip asserts that they agree)
constexpr int kSpatialFilterBox = 2;        // SF_BOX
constexpr int kNeeKickstart = 1;            // NEE_KICKSTART
constexpr unsigned int kBlock = 256;        // PPG_BLOCK
constexpr unsigned int kDenseChunk = 256;   // PPG_DCHUNK
constexpr unsigned int kAdamLeafShift = 40; // PPG_ADAM_LEAF_SHIFT

// Adam records: positions are known in advance unless one vertex can make several records (box spatial filter) or records are made
// while the paths are still being traced (the direct-light vertex of nee = kickstart)
inline bool recordPositionsKnown(int spatialFilter, bool doNee, int nee) { return spatialFilter != kSpatialFilterBox && !(doNee && nee == kNeeKickstart); }

// side streams may be used (kernel timing wants every kernel alone on the context's stream)
inline bool sideStreamsAllowed(bool timerOn, bool tuneNoOverlap) { return !timerOn && !tuneNoOverlap; }

// key bit of "a splat only" in a round committed through records: just above the leaf bits (every leaf index is below the all-ones pattern of a hole)
inline unsigned int adamFlagShift(size_t streeNodes) {
    unsigned int leafBits = 1;
    while ((1u << leafBits) <= (unsigned int)streeNodes) ++leafBits;
    return kAdamLeafShift + leafBits;
}

struct BatchFacts {
    unsigned int paths = 0;               // of this batch
    int maxDepth = -1;                    // < 0: unbounded paths
    bool isFinalIter = false, adamRound = false;
    bool last = true;                     // no batch follows at once
    int spatialFilter = 0, nee = 0;       // recordPositionsKnown
    bool doNee = false;
    bool timerOn = false;
    bool tuneNoOverlap = false, tuneNoSortedCommit = false;
    int tuneSplitDepth = 0;
    unsigned int tailThreshold = 0, tailMin = 0, tailDiv = 1;
    int deferDepthAdam = 0;
    size_t streeNodes = 0;
    bool prevPendingWithRecords = false;  // the previous straggler set is pending and leaves optimiser records
    unsigned int prevStragglers = 0;      // paths of that set
    int maxVertices = 0;
};

struct BatchPlan {
    bool adamFast;            // a round of the optimiser whose record positions are known in advance
    unsigned int stopBelow;   // live paths below which the wavefront stops (unbounded paths: k_tail takes over; bounded paths: nothing is left)
    bool tail;                // persistent threads finish the survivors (k_tail)
    bool commit;              // the recorded vertices go into the building tree
    bool fastRound;           // adamFast with paths: positions = exclusive scan of the vertex counts
    bool deferRecords;        // the stragglers' records are applied one round late (include/ppg.h "STRAGGLERS": part of the result)
    unsigned int deferDepth;  // depth at which k_tail hands its stragglers over (0: it runs every path to its end)
    bool splitTail;           // deferDepth > 0
    bool beside;              // side streams may be used
    bool overlap;             // k_commit of the paths that HAVE ended when k_tail takes over runs beside it, a second one takes the rest
    unsigned int adamFlagShift;
    bool sortedCommit;        // records, the optimiser's sort, splats D-tree by D-tree instead of k_commit's global atomics
    size_t nDeferredIn;       // record positions of the PREVIOUS round's stragglers, applied with this round's: behind its own
};

inline BatchPlan planBatch(const BatchFacts &f) {
    BatchPlan p{};
    const bool unbounded = f.maxDepth < 0;
    p.adamFast = f.adamRound && recordPositionsKnown(f.spatialFilter, f.doNee, f.nee);
    p.stopBelow = unbounded ? (f.tailThreshold ? f.tailThreshold : std::max(f.tailMin, f.paths / f.tailDiv)) : 1u;
    p.tail = unbounded && f.paths > 0;
    p.commit = !f.isFinalIter && f.paths > 0;
    p.fastRound = p.adamFast && f.paths > 0;
    p.beside = sideStreamsAllowed(f.timerOn, f.tuneNoOverlap);
    // In a round of the optimiser whose record positions are known the hand-over depth is part of the result; elsewhere it is scheduling
    // only, and worth it only when another batch follows at once.
    p.deferRecords = p.adamFast && unbounded;
    p.deferDepth = !p.tail ? 0u : (p.deferRecords ? (unsigned int)f.deferDepthAdam : ((!f.last && !f.adamRound && p.beside) ? (unsigned int)f.tuneSplitDepth : 0u));
    p.splitTail = p.deferDepth > 0;
    // (with a split tail the two-phase commit is needed anyway: the hand-over must be known before the tail runs)
    p.overlap = p.tail && p.commit && (p.beside || p.splitTail);
    p.adamFlagShift = adamFlagShift(f.streeNodes);
    // (the flag needs a key bit above the leaf: an S-tree of 2^23 nodes or more — never seen — commits with k_commit)
    p.sortedCommit = p.adamFast && !f.tuneNoSortedCommit && p.adamFlagShift < 63u;
    p.nDeferredIn = (p.adamFast && f.prevPendingWithRecords) ? (size_t)f.prevStragglers * (size_t)f.maxVertices : 0;
    return p;
}

// The previous batch's survival curve: live paths after each wavefront bounce it ran.  It sizes the schedule of the next batch.
struct SurvivalCurve {
    int bounces = 0;
    unsigned int paths = 0, live[64] = {};
};

// Wavefront bounces to LAUNCH for a batch (nothing is read back in between: the device raises a stop flag when the live count has fallen below
// stopBelow, and the kernels launched beyond that point return at once).  Bounded paths run maxDepth bounces.  Unbounded paths:
// live(b) of this batch ~ (live(b) / paths of the previous batch) * paths of this one; beyond what was observed, the last ratio.
// tuneBulkBounces >= 0 fixes the number (PPG_BULK_BOUNCES); margin: bounces beyond the predicted need (PPG_BOUNCE_MARGIN).
inline int planBounces(const SurvivalCurve &c, unsigned int paths, unsigned int stopBelow, int maxDepth, int tuneBulkBounces, int margin, bool adamFast, int deferDepthAdam) {
    if (maxDepth >= 0) return maxDepth;
    int maxBounces;
    if (tuneBulkBounces >= 0) maxBounces = std::min(64, tuneBulkBounces);
    else {
        int need = 8;
        if (c.bounces > 0 && c.paths > 0) {
            const double scale = (double)paths / (double)c.paths;
            need = -1;
            for (int b = 0; b < c.bounces; ++b) if (c.live[b] * scale < stopBelow) { need = b + 1; break; }
            if (need < 0) {
                double live = c.live[c.bounces - 1] * scale;
                const double before = c.bounces > 1 ? c.live[c.bounces - 2] : (double)c.paths;
                const double ratio = std::min(0.97, std::max(0.5, before > 0 ? c.live[c.bounces - 1] / before : 0.9));
                need = c.bounces;
                while (live >= stopBelow && need < 64) { live *= ratio; ++need; }
            }
        }
        maxBounces = std::max(1, std::min(64, need + margin));
        // (a batch smaller than the hand-over threshold stops after its first bounce whatever happens: no margin — every launch beyond the
        // stop returns at once, but three kernels and two small ones per bounce are still 30 us of launches, 0.5 ms in a first batch)
        if (paths < stopBelow) maxBounces = 1;
    }
    // (a round whose stragglers' records are deferred: a path alive after wavefront bounce b has depth b, and which paths are
    // stragglers is decided where k_tail takes them — never beyond the depth of the rule, include/ppg.h "STRAGGLERS")
    if (adamFast) maxBounces = std::min(maxBounces, std::max(1, deferDepthAdam));
    return maxBounces;
}

// live[b]: paths alive after bounce b of the batch just rendered, bouncesRun of them launched.  Keeps the curve up to the bounce that crossed
// stopBelow; returns how many bounces that is.
inline int observeBounces(SurvivalCurve &c, const unsigned int *live, int bouncesRun, unsigned int paths, unsigned int stopBelow) {
    int ran = bouncesRun;
    for (int b = 0; b < bouncesRun; ++b) if (live[b] < stopBelow) { ran = b + 1; break; }
    c.bounces = ran; c.paths = paths;
    for (int b = 0; b < ran; ++b) c.live[b] = live[b];
    return ran;
}

// Workgroups of a batch's wavefront kernels.  A batch of a few million paths runs faster on fewer, larger queue slices (ray replacement and
// the slice sort have more to work with, fewer half-empty workgroups per launch), the largest launches of a long render on more — so the grid
// follows the batch.  Slices are sized for the largest batch on nBlocks workgroups: a smaller grid is taken only if this batch's slices still fit.
inline int wavefrontGrid(int nBlocks, int tuneBlocksSmall, size_t tuneSmallPaths, unsigned int paths, unsigned int queueCap) {
    if (tuneBlocksSmall > 0 && tuneBlocksSmall < nBlocks && (size_t)paths <= tuneSmallPaths) {
        const size_t chunks = ((size_t)paths + kDenseChunk - 1) / kDenseChunk;
        if (((chunks + (size_t)tuneBlocksSmall - 1) / (size_t)tuneBlocksSmall) * kDenseChunk <= (size_t)queueCap) return tuneBlocksSmall;
    }
    return nBlocks;
}

struct TailShape { int grid; unsigned int laneLimit; };  // workgroups of a k_tail launch, paths a wave takes at a time

// k_tail behind the wavefront.  Its persistent workgroups hold their registers until their last path has ended: no more of them than fit the GPU
// at once.  Fewer paths than lanes — a rank's share of a small round, a round over one group of blocks —: dealt THINLY, the same number of
// lanes in every wave, instead of 64 to the first waves and none to the rest (a wave's bounce costs the union of its lanes' branches and its
// longest traversal, and idle SIMDs cost nothing).  handedPaths: how many paths the launch will find, when the host knows — 0 = unknown.
inline TailShape tailShape(int wavefrontGrid, int tuneTailBlocks, size_t handedPaths) {
    const int grid = std::min(wavefrontGrid, tuneTailBlocks ? tuneTailBlocks : 1024);
    const size_t waves = (size_t)grid * (kBlock / 64);
    return {grid, handedPaths ? (unsigned int)std::max<size_t>(1, std::min<size_t>(64, (handedPaths + waves - 1) / waves)) : 64u};
}
// k_tail of n stragglers: as many waves as there are stragglers while the GPU has room for them (a lone path's bounce is 12 us, 64 in one wave 120)
inline TailShape stragglerShape(unsigned int n) {
    const unsigned int waves = 1024u * (kBlock / 64u);
    const unsigned int laneLimit = std::max(1u, std::min(64u, (n + waves - 1u) / waves));
    return {(int)std::max(1u, std::min(1024u, (n + laneLimit * (kBlock / 64u) - 1u) / (laneLimit * (kBlock / 64u)))), laneLimit};
}

// The pinned block a batch's counts are read back into.
struct RoundReadback {
    unsigned int live[64];                  // live paths after each wavefront bounce
    unsigned int slowCount, slowOverflow;   // a round whose positions are NOT known: records made, overflow word (one 8-byte copy)
    unsigned int sumBase, lastNv;           // a fast round: exclusive scan and vertex count of the last path — their sum is the round's own positions
    unsigned long long handed;              // paths handed to k_tail (a split tail)
    unsigned long long stragglers;          // alive at the hand-over depth
};
static_assert(offsetof(RoundReadback, slowOverflow) == offsetof(RoundReadback, slowCount) + 4, "one 8-byte copy fills both");

// which paths a commit launch takes
enum class CommitSet {
    All,    // every path
    Ended,  // paths not flagged as stragglers
    List    // the paths of the dense list
};

}  // namespace ppg_plan
