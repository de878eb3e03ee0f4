"""The shared float math (include/ppg_detmath.h, ppg_rng.h) ON THE DEVICE, where the contract "GPU equals oracle, bit for bit" is made:

  * every one-argument op over ALL 2^32 float patterns, in the module of every kernel family (each compiles its own copy, and its own
    out-of-line dm_sincos / dm_atan2 / dm_exp / dm_log: via = 1), as 256 block checksums against tests/golden/detmath_exhaustive.json —
    which the oracle wrote (tools/make_detmath_golden.py) and which two blocks per op tie to the oracle built here;
  * the two-argument ops element for element against the oracle: the pow and atan2 grids of test_detmath.py, the cross product of the
    special values, 2^22 random 64-bit words through the fixed-point conversions and 2^22 sampler words;
  * the same through clang's host pass (family = -1), the compiler behind the tables csrc/ppg_scene_build.h bakes;
  * the hooks' refusals.

The ops, their domains and the checksum are those of include/ppg_mathcheck.h; the hooks are ppg_debug_math_eval / ppg_debug_math_checksum
(include/ppg_testhooks.h).  A checksum that differs is followed up: the block is evaluated input by input on both sides and the first
input that differs is reported with both bit patterns.
"""
import numpy as np
import pytest

from conftest import CBOX_PROPS
from test_detmath import CPU_BLOCKS, G, golden_checksums

f32, u32 = np.float32, np.uint32
pytestmark = pytest.mark.gpu
FAMILIES = (0, 1, 2, 3, 4, 5)  # csrc/ppg_device.h: base, shapes, ext, coat, blend, lobes
HOST = -1                      # the library's host code
HAS_DM = {"sincos", "atan2", "exp", "log", "pow", "acos", "tan"}  # ppg_mathcheck_has_dm
PPG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def engine():
    import ppg_host
    e = ppg_host.Engine.hip(**dict(CBOX_PROPS, budget=4))  # no scene: the hooks need none
    yield e
    e.close()


def canon(bits):
    bits = np.asarray(bits, u32)
    return np.where((bits & 0x7fffffff) > 0x7f800000, u32(0x7fc00000), bits)


def first_difference(engine, lib, family, via, name, block):
    """the first input of `block` at which the device (or host pass) and the oracle differ, as text"""
    patterns = (np.arange(1 << 24, dtype=np.int64) | (block << 24)).astype(u32)
    d = engine.debug_math_eval(family, via, G.OP[name], patterns)
    o = G.oracle_eval(lib, G.OP[name], patterns)
    floats = name not in ("to_fixed", "to_sfixed")
    for k in range(2):
        dk, ok = (canon(d[k]), canon(o[k])) if floats else (d[k], o[k])
        bad = np.flatnonzero(dk != ok)
        if bad.size:
            i = int(bad[0])
            return "input 0x%08x (%r), output %d: family %d via %d gives 0x%08x, the oracle 0x%08x; %d inputs of the block differ" % (
                patterns[i], float(patterns[i:i + 1].view(f32)[0]), k, family, via, d[k][i], o[k][i], bad.size)
    return "the checksums differ but no single input does"


def check_blocks(engine, lib, family, via, name, first, got):
    want = golden_checksums(name)[first:first + got.size]
    bad = np.flatnonzero(got != want)
    if bad.size:
        block = first + int(bad[0])
        pytest.fail("%s: %d of %d blocks differ from the golden file, the first is 0x%02x: %s" % (
            name, bad.size, got.size, block, first_difference(engine, lib, family, via, name, block)))


EXHAUSTIVE = [(name, via) for name in G.UNARY for via in ((0, 1) if name in HAS_DM else (0,))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,via", EXHAUSTIVE, ids=["%s-via%d" % c for c in EXHAUSTIVE])
def test_every_float_pattern_in_every_family_module(engine, oracle_lib, name, via, family):
    got = engine.debug_math_checksum(family, via, G.OP[name], 0, 256)
    check_blocks(engine, oracle_lib, family, via, name, 0, got)


@pytest.mark.parametrize("name", G.UNARY)
def test_golden_file_is_the_oracle_built_here(oracle_lib, name):
    want = golden_checksums(name)
    for k in (0x3f, 0x80):  # 1.0's block; -0, the negative denormals and the smallest negative normals
        assert G.oracle_checksum(oracle_lib, G.OP[name], k, 1)[0] == want[k], "stale golden file: %s block 0x%02x" % (name, k)


@pytest.mark.parametrize("name", G.UNARY)
def test_clangs_host_pass_on_golden_blocks(engine, oracle_lib, name):
    for k in CPU_BLOCKS:
        check_blocks(engine, oracle_lib, HOST, 0, name, k, engine.debug_math_checksum(HOST, 0, G.OP[name], k, 1))


# ---- the ops of two arguments, element for element -------------------------------------------------------------------------------------
FLT_MAX, FLT_MIN, DENORM = f32(3.4028235e38), f32(1.17549435e-38), f32(1e-42)
SPECIAL = np.array([0.0, -0.0, DENORM, -DENORM, 1.0, -1.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN], f32)


def special_pairs():
    a, b = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")
    return a.ravel(), b.ravel()


def _inputs(name):
    rng = np.random.RandomState(20240611)
    sa, sb = special_pairs()
    if name == "atan2":
        y, x = G.atan2_grid()
        return np.concatenate([y, sa]), np.concatenate([x, sb])
    if name == "pow":
        x, y = G.pow_grid()
        return np.concatenate([x, sa]), np.concatenate([y, sb])
    if name == "powi":  # bases around 1 (Adam's betas), far from it and special; every exponent of the domain, and some outside it
        base = np.concatenate([np.linspace(0.5, 1.001, 230, dtype=f32), SPECIAL, np.array([0.9, 0.999, 2.0, -0.999, 1e-20, 1e20], f32)])
        n = np.concatenate([np.arange(4096, dtype=f32), np.array([0.5, 4095.5, 4096.0, -1.0, np.nan, np.inf], f32)])
        a, b = np.meshgrid(base, n, indexing="ij")
        return a.ravel(), b.ravel()
    if name == "rand":  # the key comes from the element's index; dimensions small, large, fractional and outside the domain
        dim = np.concatenate([rng.randint(0, 64, 1 << 21), rng.randint(0, 1 << 32, (1 << 21) - 8, dtype=np.int64)]).astype(f32)
        dim = np.concatenate([dim, np.array([0.5, -0.5, -1.0, 4294967040.0, 4294967296.0, np.nan, np.inf, 1073741824.0], f32)])
        return np.zeros(dim.size, f32), dim
    if name == "rand_path":  # (pixel, seed << 16 | sample << 4 | dim) words
        return rng.randint(0, 1 << 32, 1 << 22, dtype=np.int64).astype(u32), rng.randint(0, 1 << 32, 1 << 22, dtype=np.int64).astype(u32)
    if name in ("from_fixed", "from_sfixed"):  # random 64-bit words, words of every length, and the ends of the range
        w = (rng.randint(0, 1 << 32, 1 << 22, dtype=np.int64).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 1 << 32, 1 << 22, dtype=np.int64).astype(np.uint64)
        half = 1 << 21
        w[:half] >>= (np.arange(half) % 64).astype(np.uint64)  # (the second half stays fully random)
        lo, hi = (w & np.uint64(0xffffffff)).astype(u32), (w >> np.uint64(32)).astype(u32)
        edge_lo = np.array([0, 1, 0xffffffff, 0, 0xffffffff, 0, 0xffffff80, 0x00000080], u32)
        edge_hi = np.array([0, 0, 0, 0x80000000, 0xffffffff, 0x7fffffff, 0x7fffffff, 0x00000001], u32)
        return np.concatenate([lo, edge_lo]), np.concatenate([hi, edge_hi])
    raise KeyError(name)


BINARY = ("atan2", "pow", "powi", "rand", "rand_path", "from_fixed", "from_sfixed")
_cache = {}


def binary_case(lib, name):
    """(a, b, the oracle's canonicalised results): computed once per op and left unchanged"""
    if name not in _cache:
        a, b = _inputs(name)
        o = canon(G.oracle_eval(lib, G.OP[name], a, b)[0])
        for v in (a, b, o):
            v.setflags(write=False)
        _cache[name] = (a, b, o)
    return _cache[name]


BINARY_CASES = ([(name, via, family) for name in BINARY for via in ((0, 1) if name in HAS_DM else (0,)) for family in FAMILIES]
                + [(name, 0, HOST) for name in BINARY])  # (the host has no dm_ copies: test_refusals)


@pytest.mark.parametrize("name,via,family", BINARY_CASES, ids=["%s-via%d-family%d" % c for c in BINARY_CASES])
def test_two_argument_ops_element_for_element(engine, oracle_lib, name, via, family):
    a, b, want = binary_case(oracle_lib, name)
    got = canon(engine.debug_math_eval(family, via, G.OP[name], a, b)[0])
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        ab, bb = np.ascontiguousarray(a[i:i + 1]).view(u32)[0], np.ascontiguousarray(b[i:i + 1]).view(u32)[0]
        pytest.fail("%s family %d via %d: %d of %d elements differ, the first at index %d, a = 0x%08x, b = 0x%08x: 0x%08x, the oracle 0x%08x" % (
            name, family, via, bad.size, want.size, i, ab, bb, got[i], want[i]))


def test_refusals(engine):
    import ppg_host
    atan, to_fixed, sincos, pow_ = G.OP["atan"], G.OP["to_fixed"], G.OP["sincos"], G.OP["pow"]
    x = np.ones(4, f32)
    bad = [(0, 0, 17), (0, 0, -1), (6, 0, sincos), (-2, 0, sincos), (0, 1, atan), (0, 1, to_fixed), (0, 2, sincos), (0, -1, sincos), (HOST, 1, sincos)]
    for family, via, op in bad:
        for call in (lambda: engine.debug_math_eval(family, via, op, x), lambda: engine.debug_math_checksum(family, via, op, 0, 1)):
            with pytest.raises(ppg_host.PPGError) as err:
                call()
            assert err.value.code == PPG_ERR_INVALID and "ppg_debug_math" in str(err.value), (family, via, op)
    for first, n in ((255, 2), (257, 0)):
        with pytest.raises(ppg_host.PPGError) as err:
            engine.debug_math_checksum(0, 0, sincos, first, n)
        assert err.value.code == PPG_ERR_INVALID
    with pytest.raises(ppg_host.PPGError) as err:  # an op of two arguments has no block checksum
        engine.debug_math_checksum(0, 0, pow_, 0, 1)
    assert err.value.code == PPG_ERR_INVALID
    # the context is still usable
    assert engine.debug_math_checksum(0, 0, sincos, 0x3f, 1)[0] == golden_checksums("sincos")[0x3f]
    s, c = engine.debug_math_eval(0, 1, sincos, np.zeros(3, f32))
    assert list(s.view(f32)) == [0.0] * 3 and list(c.view(f32)) == [1.0] * 3
