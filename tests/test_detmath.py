"""The shared numerical contract (include/ppg_detmath.h, ppg_rng.h) on the host: against numpy's float64 functions, and against the
exhaustive sweep of all 2^32 float patterns recorded in tests/golden/detmath_exhaustive.json (tools/make_detmath_golden.py).

Tolerances are stated in ulps of the result / absolute error; the point of these functions is not libm accuracy but bit-reproducibility
across x86-64 and gfx950, which tests/test_detmath_gpu.py checks exhaustively, per kernel-family module, against the same golden file.
The ops, their domains and the block checksum are those of include/ppg_mathcheck.h."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_detmath_golden", os.path.join(_ROOT, "tools", "make_detmath_golden.py"))
G = importlib.util.module_from_spec(_spec)  # the op numbers, accuracy domains, error measures and grids the golden file was made with
_spec.loader.exec_module(G)
GOLDEN = json.load(open(os.path.join(_ROOT, "tests", "golden", "detmath_exhaustive.json")))
f32, u32 = np.float32, np.uint32


def _eval(lib, op, a, b=None):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), np.float32)
    o0, o1 = np.zeros_like(a), np.zeros_like(a)
    fp = C.POINTER(C.c_float)
    rc = lib.ppgo_math_eval(op, C.c_uint32(a.size), a.ctypes.data_as(fp), b.ctypes.data_as(fp), o0.ctypes.data_as(fp), o1.ctypes.data_as(fp))
    assert rc == 0
    return o0, o1


def test_sincos(oracle_lib):
    x = np.linspace(-3.2, 7.0, 400001, dtype=np.float32)  # phi ranges used: [-pi/4, 3pi/4] and [0, 2pi]
    s, c = _eval(oracle_lib, 0, x)
    assert np.abs(s - np.sin(x.astype(np.float64))).max() < 1.5e-7
    assert np.abs(c - np.cos(x.astype(np.float64))).max() < 1.5e-7


def test_atan2(oracle_lib):
    rng = np.random.RandomState(1)
    y, x = rng.randn(200000).astype(np.float32), rng.randn(200000).astype(np.float32)
    a, _ = _eval(oracle_lib, 1, y, x)
    assert np.abs(a - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 4e-7  # < 2 ulp at pi
    a, _ = _eval(oracle_lib, 1, np.array([0, 1, -1, 0], np.float32), np.array([0, 0, 0, -1], np.float32))
    assert np.allclose(a, [0, np.pi / 2, -np.pi / 2, np.pi], atol=3e-7)
    # the signed zeros of C99 F.9.1.4: the pole direction (-0, +-0, +-1) goes to phi = +-pi in the reference's dirToCanonical, not to 0
    y0, x0 = np.array([0.0, -0.0, 0.0, -0.0], np.float32), np.array([0.0, 0.0, -0.0, -0.0], np.float32)
    a, _ = _eval(oracle_lib, 1, y0, x0)
    want = np.arctan2(y0, x0)
    assert np.array_equal(np.signbit(a), np.signbit(want)) and np.abs(a - want).max() < 3e-7


def test_exp(oracle_lib):
    x = np.linspace(-21, 21, 100001, dtype=np.float32)
    e, _ = _eval(oracle_lib, 2, x)
    ref = np.exp(x.astype(np.float64))
    assert (np.abs(e - ref) / ref).max() < 3e-7


def test_fixed_point_round_trip(oracle_lib):
    v = np.array([0.0, 1.0, 0.5, 0.3, 123456.789, 2.0 ** -25, 3 * 2.0 ** -25, 1e-9, 4.0e6], np.float32)
    r, _ = _eval(oracle_lib, 3, v)
    assert np.all(np.abs(r - v) <= 2.0 ** -25 + 1e-7 * v)  # resolution 2^-24, round-to-nearest-even
    assert r[0] == 0 and r[1] == 1 and r[2] == 0.5 and r[5] == 0.0 and r[6] == np.float32(2.0 ** -24 * 2)


def test_powi(oracle_lib):
    n = np.arange(0, 4000, 7).astype(np.float32)
    p, _ = _eval(oracle_lib, 5, np.full_like(n, 0.999), n)
    assert np.allclose(p, np.float64(np.float32(0.999)) ** n.astype(np.float64), rtol=1e-4)  # error grows ~ n * 2^-24; only feeds Adam's bias correction (GP:100)


def test_adam_learning_rate_is_the_references_double_expression(oracle_lib):
    """GP:100: learningRate * std::sqrt(1 - std::pow(beta2, iter)) / (1 - std::pow(beta1, iter)) — std::pow(float, int) promotes to double, so
    the reference evaluates it in double and rounds once (the float powers of round 4 were 3e-5 off at iter = 2).  The shared
    function must give that float: equal to numpy's double evaluation rounded to float, up to a rounding tie (none in this range)."""
    it = np.arange(1, 20001, dtype=np.float32)
    lr, _ = _eval(oracle_lib, 9, it)
    b1, b2, l0 = np.float64(np.float32(0.9)), np.float64(np.float32(0.999)), np.float64(np.float32(0.01))
    ref = (l0 * np.sqrt(1 - b2 ** it.astype(np.float64)) / (1 - b1 ** it.astype(np.float64))).astype(np.float32)
    assert np.array_equal(lr, ref)
    big = np.array([1 << 20, 1 << 24, (1 << 24) - 1], np.float32)  # the iteration count keeps growing over a render
    lr, _ = _eval(oracle_lib, 9, big)
    assert np.array_equal(lr, np.full(3, np.float32(0.01)))


def test_rng_uniform(oracle_lib):
    dims = np.tile(np.arange(8, dtype=np.float32), 50000)
    u, _ = _eval(oracle_lib, 4, dims, dims)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 2e-3 and abs(u.var() - 1 / 12) < 1e-3
    per_dim = u.reshape(-1, 8)
    assert np.abs(np.corrcoef(per_dim.T) - np.eye(8)).max() < 0.02  # dimensions are decorrelated


def test_log_and_pow(oracle_lib):
    x = np.exp(np.linspace(-30, 30, 200001)).astype(np.float32)
    l, _ = _eval(oracle_lib, 6, x)
    ref = np.log(x.astype(np.float64))
    assert np.abs(l - ref).max() < 2.5e-6 and (np.abs(l - ref) / np.maximum(np.abs(ref), 1e-3)).max() < 3e-7 * 40  # <= 2 ulp of the result
    l, _ = _eval(oracle_lib, 6, np.array([1.0, 0.0, -1.0], np.float32))
    assert l[0] == 0.0 and l[1] == -np.inf and np.isnan(l[2])
    rng = np.random.RandomState(2)
    a = rng.uniform(1e-6, 1.0, 100000).astype(np.float32); b = rng.uniform(0.3, 1.1, 100000).astype(np.float32)  # pow(1 - u, fit), microfacet.h:596
    p, _ = _eval(oracle_lib, 7, a, b)
    ref = a.astype(np.float64) ** b.astype(np.float64)
    assert (np.abs(p - ref) / ref).max() < 2e-6


# ---- the exhaustive golden file -------------------------------------------------------------------------------------------------------
# block 0x00: +0, the positive denormals and the smallest normals; 0x3f holds 1.0; 0x7f: 2^127 .., +inf and the positive NaNs; 0xbf holds -1.0
CPU_BLOCKS = (0x00, 0x3f, 0x7f, 0xbf)


def golden_checksums(name):
    return np.array([int(c, 16) for c in GOLDEN["ops"][name]["checksums"]], np.uint64)


def golden_worst(name):
    return [float(o["worst"]) for o in GOLDEN["ops"][name]["accuracy"]["outputs"]]


@pytest.mark.parametrize("name", G.UNARY)
def test_block_checksums_match_the_golden_file(oracle_lib, name):
    want = golden_checksums(name)
    assert want.size == 256
    for k in CPU_BLOCKS:
        got = G.oracle_checksum(oracle_lib, G.OP[name], k, 1)[0]
        assert got == want[k], "%s block 0x%02x: oracle 0x%016x, golden 0x%016x" % (name, k, got, want[k])


def test_checksum_refuses_what_it_does_not_cover(oracle_lib):
    out = (C.c_uint64 * 4)()
    for op, first, n in ((1, 0, 1), (7, 0, 1), (17, 0, 1), (-1, 0, 1), (0, 255, 2), (0, 257, 0)):
        assert oracle_lib.ppgo_math_checksum(C.c_int32(op), C.c_uint32(first), C.c_uint32(n), out) != 0, (op, first, n)


@pytest.mark.parametrize("name", sorted(G.ACCURACY))
def test_accuracy_within_the_exhaustive_bound(oracle_lib, name):
    """every 256th pattern of the accuracy domain against float64 numpy: a subset cannot exceed the exhaustive maximum, so no margin"""
    bound = golden_worst(name)
    worst = [0.0] * len(bound)
    for patterns in G.accuracy_patterns(name, 256):
        for k, (e, at) in enumerate(G.worst_error(oracle_lib, name, patterns)):
            worst[k] = max(worst[k], e)
            assert e <= bound[k], "%s output %d at 0x%08x: %r above the exhaustive %r" % (name, k, at, e, bound[k])
    print(name, "worst of the subset", worst, "exhaustive", bound)
    assert all(w > 0.25 * b for w, b in zip(worst, bound))  # (and the sweep is not vacuous: the subset comes near it)


def _around(x, name):
    """the 2^16 float patterns either side of float32 x, those inside the op's accuracy domain"""
    c = int(f32(x).view(u32))
    p = np.arange(c - (1 << 16), c + (1 << 16) + 1, dtype=np.int64)
    lo, hi, both, _, _ = G.ACCURACY[name]
    mag = p & 0x7fffffff
    return p[(mag >= lo) & (mag <= hi) & (both | (p < 0x80000000))].astype(u32)


LOG2E = 1.4426950408889634
SWITCHES = (
    [("sincos", k * np.pi / 4) for k in range(1, 9)] + [("sincos", -k * np.pi / 4) for k in (1, 8)]   # the quadrant index j changes
    + [("atan", np.tan(np.pi / 8)), ("atan", np.tan(3 * np.pi / 8)), ("atan", -np.tan(np.pi / 8))]       # ppg_atan's three ranges
    + [("log", 0.70710678118654752), ("log", 1.4142135623730951), ("log", 2.0 ** -126)]                  # m < sqrt(1/2): e - 1, 2 m - 1
    + [("exp", s * h / LOG2E) for h in (0.5, 1.5, 79.5) for s in (1, -1)]                                # floor(x log2 e + 1/2) changes
)


@pytest.mark.parametrize("name,x", SWITCHES, ids=["%s@%.6g" % s for s in SWITCHES])
def test_dense_stretches_at_the_range_reduction_switches(oracle_lib, name, x):
    patterns = _around(x, name)
    assert patterns.size >= (1 << 16)
    bound = golden_worst(name)
    for k, (e, at) in enumerate(G.worst_error(oracle_lib, name, patterns)):
        assert e <= bound[k], "%s output %d at 0x%08x: %r above the exhaustive %r" % (name, k, at, e, bound[k])
    if name == "log" or name == "exp" or name == "atan":  # monotone functions: a switch of range must not step backwards by more than the error bound allows
        o = G.oracle_eval(oracle_lib, G.OP[name], np.sort(patterns.view(f32)))[0].view(f32).astype(np.float64)
        assert (np.diff(o) >= -2 * bound[0] * G.ulp_of(o[1:])).all()


def _bits(lib, name, a, b=None):
    o0, o1 = G.oracle_eval(lib, G.OP[name], np.asarray(a, f32), None if b is None else np.asarray(b, f32))
    return o0, o1


def _fbits(*values):
    return np.array(values, f32).view(u32)


PI, PI_2 = f32(np.pi), f32(np.pi / 2)
INF, NAN = f32(np.inf), f32(np.nan)


def test_exp_and_log_at_their_limits(oracle_lib):
    """ppg_exp clamps its argument to +-80 (so it never returns 0 or inf); NaN stays NaN.  ppg_log: log(+-0) = -inf, negative -> NaN, and
    +inf is read as 2^128: 128 ln 2"""
    e = _bits(oracle_lib, "exp", [-80, -80.00001, -81, -1e30, -np.inf, 80, 80.00001, 81, 1e30, np.inf, np.nan])[0]
    assert (e[:5] == e[0]).all() and (e[5:10] == e[5]).all() and np.isnan(e[10:].view(f32)).all()
    assert e[0] == f32(1.8048513e-35).view(u32) and e[5] == f32(5.5406226e+34).view(u32)
    l = _bits(oracle_lib, "log", [0.0, -0.0, -1.0, -np.inf, np.nan, -1e-45, np.inf, 1.0])[0].view(f32)
    assert l[0] == -np.inf and l[1] == -np.inf and np.isnan(l[2:6]).all() and l[7] == 0.0
    assert l[6] == f32(88.72284)
    # the consequences for ppg_pow = exp(y log x), which the lobes family's lobe_pow guards and the other call sites never reach
    p = _bits(oracle_lib, "pow", [0.0, 0.0, 1.0], [2.0, 0.0, 1e30])[0].view(f32)
    assert p[0] == f32(1.8048513e-35) and np.isnan(p[1]) and p[2] == 1.0


def test_atan_atan2_and_acos_at_their_limits(oracle_lib):
    a = _bits(oracle_lib, "atan", [np.inf, -np.inf, 0.0, -0.0, np.nan])[0]
    assert a[0] == PI_2.view(u32) and a[1] == (-PI_2).view(u32) and a[2] == 0 and np.isnan(a[4:].view(f32)).all()
    assert a[3] == 0  # atan(-0) = +0: the sign test is xx < 0
    y = [1.0, -1.0, 1.0, -1.0, np.inf, -np.inf, np.inf, np.inf, np.inf, -np.inf, 0.0, np.nan, 1.0]
    x = [np.inf, np.inf, -np.inf, -np.inf, 1.0, 1.0, -1.0, 0.0, np.inf, -np.inf, np.inf, 1.0, np.nan]
    got = _bits(oracle_lib, "atan2", y, x)[0].view(f32)
    # a finite y over an infinite x is +-0; an infinite y over a finite x is +-inf; inf / inf is NaN (C99 would say pi/4, 3pi/4)
    want = [0.0, 0.0, PI, -PI, PI_2, -PI_2, f32(-PI_2 + PI), PI_2, NAN, NAN, 0.0, NAN, NAN]
    for k, (g, w) in enumerate(zip(got, want)):
        assert (np.isnan(g) and np.isnan(w)) or g == f32(w), (k, y[k], x[k], g, w)
    assert not np.signbit(got[1])  # atan2(-1, inf): -1 / inf = -0 and atan(-0) = +0
    c = _bits(oracle_lib, "acos", [1.0, -1.0, 0.0, 1.0000001, 2.0, -1.0000001, -2.0, np.inf, -np.inf, np.nan])[0].view(f32)
    assert c[0] == 0.0 and c[1] == PI and c[2] == PI_2
    assert (c[3:5] == 0.0).all() and (c[5:7] == PI).all()  # beyond +-1 the square root's argument is clamped to 0: acos(+-1)
    assert c[7] == 0.0 and c[8] == PI and np.isnan(c[9])  # the infinities likewise: (1 - x)(1 + x) = -inf clamps to 0


def _words(lib, name, values):
    o0, o1 = _bits(lib, name, values)
    return [(int(h) << 32) | int(l) for l, h in zip(o0, o1)]


def test_fixed_point_conversions_at_their_limits(oracle_lib):
    t = _words(oracle_lib, "to_fixed", [np.nan, np.inf, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** 26, 2.0 ** 26 * (1 - 2.0 ** -24), 1.0, 0.0, -0.0,
                                        -1e-30, -1.0, -3e38, -np.inf])
    assert t[:8] == [0, 1 << 50, 0, 2, 1 << 50, (1 << 50) - (1 << 26), 1 << 24, 0]  # ties to even: 0.5 -> 0, 1.5 -> 2; the clamp at 2^26
    assert t[8:] == [0] * 5  # every negative input is mapped to 0 before the cast
    s = _words(oracle_lib, "to_sfixed", [np.nan, np.inf, -np.inf, 2.0 ** 40, -(2.0 ** 40), 3e38, 0.5 * 2.0 ** -20, 1.5 * 2.0 ** -20, 2.5 * 2.0 ** -20,
                                         -1.5 * 2.0 ** -20, -0.5 * 2.0 ** -20, 1.0, -1.0])
    two64 = 1 << 64
    assert s == [1 << 60, 1 << 60, two64 - (1 << 60), 1 << 60, two64 - (1 << 60), 1 << 60, 0, 2, 2, two64 - 2, 0, 1 << 20, two64 - (1 << 20)]
    # (NaN has no sign the comparison x < 0 sees: +2^40)
    lo = np.array([0, 1, 0xffffffff, 0, 0xffffffff], u32)
    hi = np.array([0, 0, 0, 1 << 18, 0xffffffff], u32)
    assert list(G.oracle_eval(oracle_lib, G.OP["from_fixed"], lo, hi)[0].view(f32)) == [0.0, f32(2.0 ** -24), 256.0, f32(2.0 ** 26), f32(2.0 ** 40)]
    assert list(G.oracle_eval(oracle_lib, G.OP["from_sfixed"], lo, hi)[0].view(f32)) == [0.0, f32(2.0 ** -20), 4096.0, f32(2.0 ** 30), f32(-(2.0 ** -20))]


def test_inputs_outside_a_domain_are_not_evaluated(oracle_lib):
    """include/ppg_mathcheck.h: sincos and tan beyond 2^30 (and NaN), powi outside [0, 4096), the learning rate outside [1, 2^24]"""
    for name, a, b in (("sincos", [2.0 ** 30 * 1.0001, -np.inf, np.nan], None), ("tan", [1e10], None), ("powi", [2.0, 2.0, 2.0], [-1.0, 4096.0, np.nan]),
                       ("adam_learning_rate", [0.0, 0.99, 2.0 ** 24 + 2, np.nan], None)):
        o0, o1 = _bits(oracle_lib, name, a, b)
        assert not o0.any() and not o1.any(), name
    s, c = _bits(oracle_lib, "sincos", [2.0 ** 30, -(2.0 ** 30)])
    # the last supported argument: evaluated, finite — and useless: the three-part reduction is exact only while |x| 4/pi < 2^13 or so, and
    # beyond it the "sine" leaves [-1, 1] altogether
    assert np.isfinite(s.view(f32)).all() and np.isfinite(c.view(f32)).all() and np.abs(s.view(f32)).min() > 1e6


def test_pow_grid_within_the_measured_bound(oracle_lib):
    x, y = G.pow_grid()
    e, ok = G.pow_errors(G.oracle_eval(oracle_lib, G.OP["pow"], x, y)[0], x, y)
    assert ok.sum() == GOLDEN["pow"]["pairs_compared"]
    assert e.max() <= float(GOLDEN["pow"]["worst"])


def test_atan2_grid_within_the_measured_bound(oracle_lib):
    y, x = G.atan2_grid()
    e = G.atan2_errors(G.oracle_eval(oracle_lib, G.OP["atan2"], y, x)[0], y, x)
    assert e.size == GOLDEN["atan2"]["pairs_compared"] == 4 * 1024 * 1024
    assert e.max() <= float(GOLDEN["atan2"]["worst"])


def test_log_on_denormals_is_defined_and_useless(oracle_lib):
    """ppg_log reads a denormal as (1 + fraction) 2^-127 (include/ppg_detmath.h): documented, and pinned by the oracle's golden vectors"""
    p = np.arange(1, 0x800000, dtype=u32)
    e = G.error(G.oracle_eval(oracle_lib, G.OP["log"], p)[0], np.log(p.view(f32).astype(np.float64)), "ulp")
    assert int((e <= 1.0).sum()) == 128 and 1.9e6 < e.max() < 2.1e6 and int(e.argmax()) == 0


def test_header_and_design_quote_the_golden_file():
    """the error figures of include/ppg_detmath.h's table and of DESIGN.md section 4 are the golden file's, to three digits"""
    figures = ["%.3g" % float(o["worst"]) for name in sorted(G.ACCURACY) for o in GOLDEN["ops"][name]["accuracy"]["outputs"]]
    figures += ["%.3g" % float(GOLDEN["atan2"]["worst"]), "%.3g" % float(GOLDEN["pow"]["worst"])]
    for path in (os.path.join(_ROOT, "include", "ppg_detmath.h"), os.path.join(_ROOT, "DESIGN.md")):
        text = open(path, encoding="utf-8").read()
        for f in figures:
            assert f.replace("e-08", "e-8") in text, (path, f)
