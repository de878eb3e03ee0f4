// Host-only check of csrc/ppg_batch_plan.h — what renderBatch decides about a batch — compiled with the address and undefined-behaviour
// sanitizers and run by tests/test_batch_plan.py.  No device, no context: the header alone.
//   1. planBatch against the rule it replaced (the expressions renderBatch derived inline, kept here as parentPlan) over the full product
//      of the facts, and the invariants of a plan on every case;
//   2. planBounces / observeBounces against the loop they replaced (parentBounces) over a seeded sweep of survival curves, and the cases
//      whose answer can be derived by hand;
//   3. the layout of the pinned read-back block.
#include <cstdio>

#include "../practical-path-guiding_amd/csrc/ppg_batch_plan.h"

using namespace ppg_plan;

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- 1. the rule before the plan ----
struct Inputs {  // the context fields and arguments the inline rule read
    unsigned int paths; int maxDepth; bool isFinalIter, adamRound, last; int spatialFilter, nee; bool doNee, timer, noOverlap, noSortedCommit;
    int splitDepth; unsigned int tailThreshold, tailMin, tailDiv; int deferDepthAdam; size_t snodes; bool prevPending, prevAdam; unsigned int prevN; int maxVertices;
};
BatchPlan parentPlan(const Inputs &c) {
    BatchPlan p{};
    const bool adamRound = c.adamRound, last = c.last;
    const bool adamFast = adamRound && c.spatialFilter != 2 /* SF_BOX */ && !(c.doNee && c.nee == 1 /* NEE_KICKSTART */);
    const bool unbounded = c.maxDepth < 0;
    const unsigned int stopBelow = unbounded ? (c.tailThreshold ? c.tailThreshold : std::max(c.tailMin, c.paths / c.tailDiv)) : 1u;
    const bool tail = unbounded && c.paths > 0;
    const bool commit = !c.isFinalIter && c.paths > 0;
    const bool fastRound = adamRound && adamFast && c.paths > 0;
    const bool deferRecords = adamRound && adamFast && unbounded;
    const unsigned int deferDepth = !tail ? 0u : (deferRecords ? (unsigned int)c.deferDepthAdam : ((!last && !adamRound && !c.timer && !c.noOverlap) ? (unsigned int)c.splitDepth : 0u));
    const bool splitTail = deferDepth > 0;
    const bool beside = !c.timer && !c.noOverlap;
    const bool overlap = tail && commit && (beside || splitTail);
    unsigned int flagShift;
    {
        unsigned int leafBits = 1;
        while ((1u << leafBits) <= (unsigned int)c.snodes) ++leafBits;
        flagShift = 40 /* PPG_ADAM_LEAF_SHIFT */ + leafBits;
    }
    const bool sortedCommit = adamRound && adamFast && !c.noSortedCommit && flagShift < 63u;
    const size_t nDeferredIn = (adamRound && adamFast && c.prevPending && c.prevAdam) ? (size_t)c.prevN * (size_t)c.maxVertices : 0;
    p.adamFast = adamFast; p.stopBelow = stopBelow; p.tail = tail; p.commit = commit; p.fastRound = fastRound; p.deferRecords = deferRecords;
    p.deferDepth = deferDepth; p.splitTail = splitTail; p.beside = beside; p.overlap = overlap; p.adamFlagShift = flagShift; p.sortedCommit = sortedCommit;
    p.nDeferredIn = nDeferredIn;
    return p;
}
BatchFacts factsOf(const Inputs &c) {
    BatchFacts f;
    f.paths = c.paths; f.maxDepth = c.maxDepth; f.isFinalIter = c.isFinalIter; f.adamRound = c.adamRound; f.last = c.last;
    f.spatialFilter = c.spatialFilter; f.nee = c.nee; f.doNee = c.doNee; f.timerOn = c.timer; f.tuneNoOverlap = c.noOverlap; f.tuneNoSortedCommit = c.noSortedCommit;
    f.tuneSplitDepth = c.splitDepth; f.tailThreshold = c.tailThreshold; f.tailMin = c.tailMin; f.tailDiv = c.tailDiv; f.deferDepthAdam = c.deferDepthAdam;
    f.streeNodes = c.snodes; f.prevPendingWithRecords = c.prevPending && c.prevAdam; f.prevStragglers = c.prevN; f.maxVertices = c.maxVertices;
    return f;
}
bool samePlan(const BatchPlan &a, const BatchPlan &b) {
    return a.adamFast == b.adamFast && a.stopBelow == b.stopBelow && a.tail == b.tail && a.commit == b.commit && a.fastRound == b.fastRound &&
           a.deferRecords == b.deferRecords && a.deferDepth == b.deferDepth && a.splitTail == b.splitTail && a.beside == b.beside && a.overlap == b.overlap &&
           a.adamFlagShift == b.adamFlagShift && a.sortedCommit == b.sortedCommit && a.nDeferredIn == b.nDeferredIn;
}

void checkPlans() {
    unsigned long long cases = 0, differing = 0;
    const unsigned int pathCounts[] = {0u, 5000u, 40000000u};               // none; below tailMin; above tailMin * tailDiv
    const size_t treeSizes[] = {1000, ((size_t)1 << 22) - 1, (size_t)1 << 22};  // flag bit 51; 62 (the last that fits); 63 (k_commit instead)
    for (unsigned int bits = 0; bits < (1u << 9); ++bits)
    for (int maxDepth : {-1, 3})
    for (unsigned int paths : pathCounts)
    for (int sf = 0; sf < 3; ++sf)
    for (int nee = 0; nee < 3; ++nee)
    for (int splitDepth : {0, 6})
    for (int deferDepthAdam : {1, 64})
    for (unsigned int tailThreshold : {0u, 200u})
    for (size_t snodes : treeSizes) {
        Inputs c{};
        c.isFinalIter = bits & 1; c.adamRound = bits & 2; c.last = bits & 4; c.doNee = bits & 8; c.timer = bits & 16; c.noOverlap = bits & 32;
        c.noSortedCommit = bits & 64; c.prevPending = bits & 128; c.prevAdam = bits & 256;
        c.paths = paths; c.maxDepth = maxDepth; c.spatialFilter = sf; c.nee = nee; c.splitDepth = splitDepth; c.deferDepthAdam = deferDepthAdam;
        c.tailThreshold = tailThreshold; c.tailMin = 2097152; c.tailDiv = 12; c.snodes = snodes; c.prevN = 7; c.maxVertices = 5;
        const BatchFacts f = factsOf(c);
        const BatchPlan p = planBatch(f), q = parentPlan(c);
        ++cases;
        if (!samePlan(p, q)) {
            if (++differing <= 10) printf("FAILED planBatch differs: bits %u maxDepth %d paths %u sf %d nee %d split %d defer %d threshold %u snodes %zu\n", bits, maxDepth, paths, sf, nee,
                                          splitDepth, deferDepthAdam, tailThreshold, snodes);
            ++failures;
        }
        // the invariants of a plan
        CHECK(!p.overlap || (p.tail && p.commit), "overlap needs a tail and a commit");
        CHECK(!p.splitTail || p.tail, "only a tail can be split");
        CHECK(p.splitTail == (p.deferDepth > 0), "splitTail is deferDepth > 0");
        CHECK(!f.isFinalIter || !p.commit, "a final iteration records nothing");
        CHECK(!f.timerOn || !p.beside, "kernel timing keeps every kernel on the context's stream");
        CHECK(!p.sortedCommit || p.adamFast, "a sorted commit needs known record positions");
        CHECK(!p.adamFast || f.adamRound, "positions are known of a round's records only");
        CHECK(!(p.deferRecords && p.tail) || p.deferDepth == (unsigned int)f.deferDepthAdam, "a round's hand-over depth is the rule's");
        CHECK(f.paths > 0 || !(p.tail || p.commit || p.fastRound), "nothing to run without paths");
        CHECK(p.nDeferredIn == 0 || (p.adamFast && f.prevPendingWithRecords), "deferred records come from a pending set with records");
        CHECK(f.maxDepth < 0 || p.stopBelow == 1u, "bounded paths run until none is left");
    }
    printf("planBatch: %llu cases compared with the inline rule, %llu differing\n", cases, differing);
}

// ---- 2. the bounce predictor before the plan ----
int parentBounces(int prevBounces, unsigned int prevPaths, const unsigned int *prevLive, unsigned int nPaths, unsigned int stopBelow, int maxDepth, int tuneBulkBounces,
                  int bounceMargin, bool adamRoundFast, int deferDepthAdam) {
    const bool unbounded = maxDepth < 0;
    int maxBounces = maxDepth;
    if (unbounded) {
        if (tuneBulkBounces >= 0) maxBounces = std::min(64, tuneBulkBounces);
        else {
            int need = 8;
            if (prevBounces > 0 && prevPaths > 0) {
                const double scale = (double)nPaths / (double)prevPaths;
                need = -1;
                for (int b = 0; b < prevBounces; ++b) if (prevLive[b] * scale < stopBelow) { need = b + 1; break; }
                if (need < 0) {
                    double live = prevLive[prevBounces - 1] * scale;
                    const double before = prevBounces > 1 ? prevLive[prevBounces - 2] : (double)prevPaths;
                    const double ratio = std::min(0.97, std::max(0.5, before > 0 ? prevLive[prevBounces - 1] / before : 0.9));
                    need = prevBounces;
                    while (live >= stopBelow && need < 64) { live *= ratio; ++need; }
                }
            }
            maxBounces = std::max(1, std::min(64, need + bounceMargin));
            if (nPaths < stopBelow) maxBounces = 1;
        }
        if (adamRoundFast) maxBounces = std::min(maxBounces, std::max(1, deferDepthAdam));
    }
    return maxBounces;
}

uint64_t rngState = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rngState = rngState * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rngState >> 33); }

void checkBounces() {
    unsigned long long cases = 0, differing = 0;
    for (int k = 0; k < 200000; ++k) {
        SurvivalCurve c;
        c.bounces = (int)(rnd() % 65);  // 0 .. 64
        c.paths = (rnd() % 8 == 0) ? 0u : 1u + rnd() % 60000000u;
        double live = c.paths;
        for (int b = 0; b < c.bounces; ++b) { live *= 0.3 + 0.699 * (rnd() % 1000) / 1000.0; c.live[b] = (unsigned int)live; }
        if (c.bounces && rnd() % 16 == 0) c.live[rnd() % (unsigned int)c.bounces] = 0;  // (a curve need not be monotone for the rule to be defined)
        const unsigned int paths = 1u + rnd() % 60000000u;
        const unsigned int stopBelow = (rnd() % 4 == 0) ? 1u + rnd() % 100u : 1u + rnd() % 4000000u;
        const int maxDepth = (rnd() % 8 == 0) ? (int)(rnd() % 20) : -1;
        const int bulk = (rnd() % 8 == 0) ? (int)(rnd() % 100) : -1;
        const int margin = (int)(rnd() % 6);
        const bool fast = rnd() % 4 == 0;
        const int deferDepthAdam = (rnd() % 2) ? 64 : (int)(rnd() % 10);
        const int got = planBounces(c, paths, stopBelow, maxDepth, bulk, margin, fast, deferDepthAdam);
        const int want = parentBounces(c.bounces, c.paths, c.live, paths, stopBelow, maxDepth, bulk, margin, fast, deferDepthAdam);
        ++cases;
        if (got != want) { ++differing; ++failures; if (differing <= 10) printf("FAILED planBounces %d, the inline rule %d (case %d)\n", got, want, k); }
        CHECK(got <= 64 || maxDepth > 64, "never more than 64 wavefront bounces of unbounded paths");
        if (maxDepth < 0 && bulk < 0) CHECK(got >= 1, "the adaptive schedule launches a bounce");  // (PPG_BULK_BOUNCES=0 asks for none)
    }
    printf("planBounces: %llu curves compared with the inline rule, %llu differing\n", cases, differing);

    const unsigned int stop = 1000u, paths = 1000000u;
    const int margin = 3;
    auto plan = [&](const SurvivalCurve &c, unsigned int n = 1000000u, int m = 3, int bulk = -1, bool fast = false, int defer = 64, int maxDepth = -1) {
        return planBounces(c, n, stop, maxDepth, bulk, m, fast, defer);
    };
    SurvivalCurve none;
    CHECK(plan(none) == 8 + margin, "no history: 8 + margin, got %d", plan(none));
    SurvivalCurve crossing;
    crossing.bounces = 5; crossing.paths = paths;
    const unsigned int lv[5] = {500000u, 250000u, 900u, 300u, 10u};
    for (int b = 0; b < 5; ++b) crossing.live[b] = lv[b];
    CHECK(plan(crossing) == 2 + 1 + margin, "a curve that crosses after bounce 2: 3 + margin, got %d", plan(crossing));
    CHECK(plan(crossing, 2 * paths) == 3 + 1 + margin, "twice the paths: 2 * 900 >= 1000, crosses after bounce 3, got %d", plan(crossing, 2 * paths));
    // beyond what was observed: the last ratio, clamped to [0.5, 0.97]
    for (const double r : {0.9, 0.995, 0.1}) {
        SurvivalCurve c;
        c.bounces = 2; c.paths = paths; c.live[0] = 800000u; c.live[1] = (unsigned int)(800000u * r);
        const double clamped = r > 0.97 ? 0.97 : (r < 0.5 ? 0.5 : (double)c.live[1] / c.live[0]);
        int need = 2;
        for (double live = c.live[1]; live >= stop && need < 64; live *= clamped) ++need;
        const int want = need + margin > 64 ? 64 : need + margin;
        CHECK(plan(c) == want, "extrapolation with ratio %g: want %d, got %d", r, want, plan(c));
    }
    {   // the clamp is what decides: 0.1 unclamped would cross at once
        SurvivalCurve c;
        c.bounces = 2; c.paths = paths; c.live[0] = 800000u; c.live[1] = 80000u;
        CHECK(plan(c, paths, 0) == 2 + 7, "80000 * 0.5^7 = 625 < 1000 <= 80000 * 0.5^6: 7 more bounces, got %d", plan(c, paths, 0));
    }
    {   // a single observed bounce: the ratio is taken against the batch's paths
        SurvivalCurve c;
        c.bounces = 1; c.paths = paths; c.live[0] = 500000u;
        CHECK(plan(c, paths, 0) == 1 + 9, "500000 * 0.5^9 = 976 < 1000: 9 more bounces, got %d", plan(c, paths, 0));
    }
    SurvivalCurve flat;  // nothing ever dies: the limit
    flat.bounces = 3; flat.paths = paths; flat.live[0] = flat.live[1] = flat.live[2] = paths;
    CHECK(plan(flat) == 64, "never above 64, got %d", plan(flat));
    CHECK(plan(crossing, 999u) == 1 && plan(none, 999u) == 1 && plan(flat, 999u) == 1, "a batch smaller than stopBelow: one bounce");
    CHECK(plan(crossing, paths, margin, 5) == 5 && plan(crossing, paths, margin, 100) == 64 && plan(crossing, 999u, margin, 7) == 7, "PPG_BULK_BOUNCES: min(64, value)");
    CHECK(plan(flat, paths, margin, -1, true, 6) == 6 && plan(flat, paths, margin, -1, true, 0) == 1 && plan(flat, paths, margin, 40, true, 6) == 6 &&
          plan(crossing, paths, margin, -1, true, 64) == 6, "a fast round: capped at max(1, deferDepthAdam)");
    CHECK(plan(flat, paths, margin, -1, false, 64, 7) == 7 && plan(none, 999u, margin, 3, true, 2, 12) == 12 && plan(none, paths, margin, -1, false, 64, 0) == 0, "bounded paths: maxDepth");
    {   // what a batch observed is what an equal batch is given
        const unsigned int device[8] = {600000u, 300000u, 100u, 0u, 0u, 0u, 0u, 0u};
        SurvivalCurve c;
        const int ran = observeBounces(c, device, 6, paths, stop);
        CHECK(ran == 3 && c.bounces == 3 && c.paths == paths && c.live[0] == 600000u && c.live[2] == 100u, "observeBounces keeps the curve up to the crossing bounce, ran %d", ran);
        CHECK(plan(c, paths, 0) == 3, "observe, then plan an equal batch: the crossing bounce, got %d", plan(c, paths, 0));
        const unsigned int alive[4] = {900000u, 800000u, 700000u, 600000u};
        CHECK(observeBounces(c, alive, 4, paths, stop) == 4 && c.bounces == 4 && c.live[3] == 600000u, "a curve that did not cross: every bounce run");
        CHECK(observeBounces(c, alive, 0, paths, stop) == 0 && c.bounces == 0 && plan(c) == 8 + margin, "no bounce run: no history");
    }
    // the grids
    CHECK(wavefrontGrid(4096, 2048, 13000000, 1000000u, 1u << 20) == 2048 && wavefrontGrid(4096, 2048, 13000000, 14000000u, 1u << 20) == 4096 &&
          wavefrontGrid(4096, 0, 13000000, 1000u, 1u << 20) == 4096 && wavefrontGrid(1024, 2048, 13000000, 1000u, 1u << 20) == 1024, "the small grid for small batches only");
    CHECK(wavefrontGrid(4096, 2048, 13000000, 2048u * 256u + 1u, 256u) == 4096 && wavefrontGrid(4096, 2048, 13000000, 2048u * 256u, 256u) == 2048, "... and only if the slices fit");
    CHECK(tailShape(2048, 0, 0).grid == 1024 && tailShape(2048, 0, 0).laneLimit == 64u && tailShape(512, 0, 0).grid == 512 && tailShape(2048, 300, 0).grid == 300, "k_tail's grid");
    CHECK(tailShape(2048, 0, 1).laneLimit == 1u && tailShape(2048, 0, 4096).laneLimit == 1u && tailShape(2048, 0, 4097).laneLimit == 2u && tailShape(2048, 0, 1u << 30).laneLimit == 64u, "k_tail's lanes per wave");
    CHECK(stragglerShape(1).grid == 1 && stragglerShape(1).laneLimit == 1u && stragglerShape(9).grid == 3 && stragglerShape(4096).grid == 1024 && stragglerShape(4096).laneLimit == 1u &&
          stragglerShape(4097).laneLimit == 2u && stragglerShape(4097).grid == 513 && stragglerShape(10000000u).laneLimit == 64u && stragglerShape(10000000u).grid == 1024, "the stragglers' grid");
}

// ---- 3. the pinned block: fields in this order, none over another, nothing beyond the allocation (sizeof(RoundReadback), allocPaths) ----
#define END_OF(f) (offsetof(RoundReadback, f) + sizeof(RoundReadback::f))
static_assert(offsetof(RoundReadback, live) == 0 && sizeof(RoundReadback::live) == 64 * 4, "the device's 64 bounce counts");
static_assert(END_OF(live) <= offsetof(RoundReadback, slowCount) && END_OF(slowCount) <= offsetof(RoundReadback, slowOverflow) &&
              END_OF(slowOverflow) <= offsetof(RoundReadback, sumBase) && END_OF(sumBase) <= offsetof(RoundReadback, lastNv) &&
              END_OF(lastNv) <= offsetof(RoundReadback, handed) && END_OF(handed) <= offsetof(RoundReadback, stragglers) && END_OF(stragglers) <= sizeof(RoundReadback),
              "no two fields overlap");
static_assert(offsetof(RoundReadback, slowOverflow) - offsetof(RoundReadback, slowCount) == 4, "the slow round's count and overflow word arrive in one 8-byte copy");
static_assert(sizeof(RoundReadback::handed) == 8 && sizeof(RoundReadback::stragglers) == 8 && offsetof(RoundReadback, handed) % 8 == 0, "64-bit device counters");

}  // namespace

int main() {
    checkPlans();
    checkBounces();
    if (failures) { printf("%d check(s) FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
