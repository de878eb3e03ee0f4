// The domain predicate of include/ppg_mathcheck.h, checked where it can be: this program is compiled with the undefined-behaviour sanitizer
// (float-cast-overflow, signed overflow, shifts) and evaluates every op on inputs INSIDE its domain — a stride through all 2^32 float
// patterns, every pattern near the values where a domain or a branch of the functions begins or ends, and the cross product of the special
// values for the ops of two arguments.  "Every C++ step is defined for this input" then means: the sanitizer stays silent.
// One exception, stated in the header: ppg_exp (and ppg_pow through it) converts a NaN argument to int on its way to a NaN result; those
// inputs are left out here and pinned by tests/test_detmath.py.  Host only; tests/test_mathcheck_domain.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/ppg_mathcheck.h"

static unsigned long long g_evaluated = 0, g_outside = 0, g_sum = 0;

static bool expArgumentIsNaN(int op, uint32_t a, uint32_t b) {
    if (op == 2) { const float x = ppg_u2f(a); return x != x; }
    if (op == 7) { const float t = ppg_u2f(b) * ppg_log(ppg_u2f(a)); return t != t; }
    return false;
}
static void one(int op, uint32_t a, uint32_t b) {
    if (!ppg_mathcheck_in_domain(op, a, b)) { ++g_outside; return; }
    if (expArgumentIsNaN(op, a, b)) return;
    uint32_t o0 = 0, o1 = 0;
    ppg_mathcheck_eval(op, a, b, &o0, &o1);
    g_sum += ppg_mathcheck_mix(a, o0, o1);
    ++g_evaluated;
}

int main() {
    // where a domain, a clamp or a branch begins or ends
    const float edges[] = {0.0f, 1.1754944e-38f, 0.41421357f, 0.70710678f, 0.78539816f, 1.0f, 1.5f, 2.4142135f, 80.0f, 4096.0f, 8192.0f, 16777216.0f,
                           67108864.0f, 1073741824.0f, 2147483648.0f, 4294967296.0f, 1.099511627776e12f, 1125899906842624.0f, 9.2233720e18f,
                           1.8446744e19f, 3.4028235e38f, __builtin_inff()};
    std::vector<uint32_t> patterns;
    for (uint64_t u = 0; u < (1ull << 32); u += 4099) patterns.push_back((uint32_t)u);
    for (float e : edges)
        for (int sign = 0; sign < 2; ++sign)
            for (int d = -4096; d <= 4096; ++d) patterns.push_back((uint32_t)((int64_t)ppg_f2u(e) + d) | (sign ? 0x80000000u : 0u));
    const uint32_t special[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x80800000u, 0x3f800000u, 0xbf800000u,
                                0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x40000000u, 0x457ff000u,
                                0x45800000u, 0x4f7fffffu, 0x4f800000u, 0xbf7fffffu, 0x3f000000u, 0xffffffffu};
    for (int op = 0; op < PPG_MATHCHECK_OPS; ++op) {
        if (ppg_mathcheck_unary(op))
            for (uint32_t u : patterns) one(op, u, 0u);
        else {
            for (uint32_t a : special)
                for (uint32_t b : special) one(op, ppg_mathcheck_arg_a(op, a, a), b);
            for (size_t k = 0; k + 1 < patterns.size(); k += 7) one(op, ppg_mathcheck_arg_a(op, (uint32_t)k, patterns[k]), patterns[patterns.size() - 1 - k]);
        }
    }
    // the predicate itself: what it must refuse
    int failed = 0;
    auto refuse = [&](int op, float a, float b) {
        if (ppg_mathcheck_in_domain(op, ppg_f2u(a), ppg_f2u(b))) { printf("FAILED: op %d accepts (%g, %g)\n", op, a, b); ++failed; }
    };
    const float nan = __builtin_nanf("");
    refuse(0, 1073741952.0f, 0); refuse(0, -__builtin_inff(), 0); refuse(0, nan, 0); refuse(12, 1e10f, 0); refuse(12, nan, 0);
    refuse(4, 0, -1.0f); refuse(4, 0, 4294967296.0f); refuse(4, 0, nan);
    refuse(5, 2.0f, -1.0f); refuse(5, 2.0f, 4096.0f); refuse(5, 2.0f, nan);
    refuse(9, 0.99999994f, 0); refuse(9, 16777218.0f, 0); refuse(9, nan, 0); refuse(9, -5.0f, 0);
    refuse(17, 1.0f, 0); refuse(-1, 1.0f, 0);
    printf("mathcheck: %llu inputs evaluated inside their domains, %llu outside and skipped, checksum %016llx\n", g_evaluated, g_outside, g_sum);
    if (failed) return 1;
    printf("all checks passed\n");
    return 0;
}
