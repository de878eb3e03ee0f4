#!/usr/bin/env python3
"""Writes tests/golden/detmath_exhaustive.json: the shared float math (include/ppg_detmath.h) swept over ALL 2^32 float patterns by the oracle.

    python tools/make_detmath_golden.py [--out FILE] [--threads N]

Per one-argument op of include/ppg_mathcheck.h (sincos, atan, acos, tan, exp, log, to_fixed, to_sfixed, adam_learning_rate):
  checksums   the 256 block checksums of ppgo_math_checksum (block k = the patterns k << 24 .. (k << 24) + 2^24 - 1, inputs outside the op's
              domain contribute nothing) — what every device module and clang's host pass must reproduce (tests/test_detmath_gpu.py)
  accuracy    the exhaustive worst error against numpy's float64 function over the op's ACCURACY domain, with the input (bit pattern) it
              occurs at: absolute for sincos on |x| <= 8192; in ulps of the float32 grid at the float64 result for atan (all finite), acos
              ([-1, 1]), tan (|x| <= 1.5), exp ([-80, 80]) and log (normal x > 0)
and, for the two-argument functions, the worst error in ulps over the pow and atan2 grids below.  tests/test_detmath.py holds a subset of
the same inputs to these figures without a margin; include/ppg_detmath.h and DESIGN.md quote them.  The file depends on the oracle and on
numpy's float64 functions only: two runs write identical files.  A few minutes on eight cores.
"""
import argparse
import ctypes as C
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "detmath_exhaustive.json")

# op numbers of include/ppg_mathcheck.h
OP = dict(sincos=0, atan2=1, exp=2, fixed_round_trip=3, rand=4, powi=5, log=6, pow=7, rand_path=8, adam_learning_rate=9, atan=10, acos=11, tan=12,
          to_fixed=13, to_sfixed=14, from_fixed=15, from_sfixed=16)
UNARY = ("sincos", "atan", "acos", "tan", "exp", "log", "to_fixed", "to_sfixed", "adam_learning_rate")


def f2u(x):
    return int(np.float32(x).view(np.uint32))


# accuracy domains: (lowest, highest) bit pattern of |x|, whether the negative patterns belong too, the float64 reference, the measure
ACCURACY = dict(
    sincos=(0, f2u(8192.0), True, (np.sin, np.cos), "abs"),
    atan=(0, 0x7f7fffff, True, (np.arctan,), "ulp"),
    acos=(0, f2u(1.0), True, (np.arccos,), "ulp"),
    tan=(0, f2u(1.5), True, (np.tan,), "ulp"),
    exp=(0, f2u(80.0), True, (np.exp,), "ulp"),
    log=(0x00800000, 0x7f7fffff, False, (np.log,), "ulp"),
)


def ulp_of(ref):
    """spacing of the float32 grid at the float64 value ref (that of the denormals below 2^-126)"""
    ref = np.abs(np.asarray(ref, np.float64))
    _, e = np.frexp(ref)  # ref = m 2^e, m in [0.5, 1)
    e = np.where(ref == 0, -126, e - 1)
    return np.ldexp(1.0, np.maximum(e, -126) - 23)


def error(got_bits, ref, measure):
    """error of the float32 results (bit patterns) against the float64 reference: absolute, or in ulps at the reference"""
    got = np.asarray(got_bits, np.uint32).view(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref)
    d = np.where(got == ref, 0.0, d)  # (inf - inf)
    return d if measure == "abs" else d / ulp_of(ref)


def oracle_eval(lib, op, a, b=None):
    """ppgo_math_eval on bit patterns (uint32 or float32 arrays) -> (out0, out1) as uint32"""
    a = np.ascontiguousarray(a)
    a = a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32, casting="same_kind")
    if b is None:
        b = np.zeros_like(a)
    b = np.ascontiguousarray(b)
    b = b.view(np.uint32) if b.dtype == np.float32 else b.astype(np.uint32, casting="same_kind")
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    o0, o1 = np.zeros_like(a), np.zeros_like(a)
    fp = C.POINTER(C.c_float)
    rc = lib.ppgo_math_eval(C.c_int32(op), C.c_uint32(a.size), a.ctypes.data_as(fp), b.ctypes.data_as(fp), o0.ctypes.data_as(fp), o1.ctypes.data_as(fp))
    assert rc == 0, rc
    return o0, o1


def oracle_checksum(lib, op, first_block, n_blocks):
    out = np.zeros(n_blocks, np.uint64)
    rc = lib.ppgo_math_checksum(C.c_int32(op), C.c_uint32(first_block), C.c_uint32(n_blocks), out.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, rc
    return out


def accuracy_patterns(name, step=1):
    """every step-th bit pattern of the op's accuracy domain, in chunks of at most 2^22"""
    lo, hi, both, _, _ = ACCURACY[name]
    for sign in ((0, 0x80000000) if both else (0,)):
        start = lo
        while start <= hi:
            stop = min(hi + 1, start + (1 << 22) * step)
            yield (np.arange(start, stop, step, dtype=np.int64) | sign).astype(np.uint32)
            start = stop + (-(stop - lo) % step)


def worst_error(lib, name, patterns):
    """(worst error per output, pattern it occurs at per output) of op `name` over the patterns"""
    _, _, _, refs, measure = ACCURACY[name]
    o = oracle_eval(lib, OP[name], patterns)
    x = patterns.view(np.float32).astype(np.float64)
    res = []
    for k, f in enumerate(refs):
        with np.errstate(all="ignore"):
            e = error(o[k], f(x), measure)
        i = int(np.argmax(e))
        res.append((float(e[i]), int(patterns[i])))
    return res


def pow_grid():
    """x: 2048 values log-spaced over [2^-40, 1], and 0; y: 2048 values log-spaced over [2^-10, 2^20], and 0; every pair"""
    x = np.exp2(-40.0 * (1.0 - np.arange(2048) / 2047.0)).astype(np.float32)
    y = np.exp2(-10.0 + 30.0 * np.arange(2048) / 2047.0).astype(np.float32)
    x = np.unique(np.concatenate([x, np.array([0.0, 1.0], np.float32)]))
    y = np.unique(np.concatenate([y, np.array([0.0], np.float32)]))
    X, Y = np.meshgrid(x, y, indexing="ij")
    return np.ascontiguousarray(X.ravel()), np.ascontiguousarray(Y.ravel())


def atan2_grid():
    """both arguments: 1024 magnitudes log-spaced over the normal range [2^-126, 2^128), with all four sign pairs"""
    m = np.exp2(-126.0 + 254.0 * np.arange(1024) / 1024.0).astype(np.float32)
    A, B = np.meshgrid(m, m, indexing="ij")
    A, B = A.ravel(), B.ravel()
    return np.ascontiguousarray(np.concatenate([A, A, -A, -A])), np.ascontiguousarray(np.concatenate([B, -B, B, -B]))


def pow_errors(got_bits, x, y):
    """ulp errors of ppg_pow where |y ln x| <= 80 (the rest of the grid is outside ppg_exp's range: 0 there), against float64"""
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        t = yd * np.log(xd)
        ok = np.abs(t) <= 80.0  # (false for x = 0: t is -inf or NaN)
        ref = np.where(ok, np.power(np.where(ok, xd, 1.0), yd), 1.0)
    return np.where(ok, error(got_bits, ref, "ulp"), 0.0), ok


def atan2_errors(got_bits, y, x):
    return error(got_bits, np.arctan2(y.astype(np.float64), x.astype(np.float64)), "ulp")


def load_oracle():
    return C.CDLL(os.path.join(ROOT, "oracle", "libppg_oracle.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    os.environ["OMP_NUM_THREADS"] = "1"  # the chunks run on Python threads; the oracle's loops stay serial inside each
    lib = load_oracle()
    doc = {"ops": {}}
    with ThreadPoolExecutor(args.threads) as pool:
        for name in UNARY:
            sums = list(pool.map(lambda k: int(oracle_checksum(lib, OP[name], k, 1)[0]), range(256)))
            entry = {"op": OP[name], "checksums": ["0x%016x" % s for s in sums]}
            if name in ACCURACY:
                parts = list(pool.map(lambda p: worst_error(lib, name, p), accuracy_patterns(name)))
                outs = []
                for k in range(len(ACCURACY[name][3])):
                    e, at = max((p[k] for p in parts), key=lambda t: (t[0], -t[1]))
                    outs.append({"worst": repr(e), "at_bits": "0x%08x" % at, "at": repr(float(np.uint32(at).view(np.float32)))})
                entry["accuracy"] = {"measure": ACCURACY[name][4], "lo_bits": "0x%08x" % ACCURACY[name][0], "hi_bits": "0x%08x" % ACCURACY[name][1],
                                     "negatives": ACCURACY[name][2], "outputs": outs}
            doc["ops"][name] = entry
            print(name, entry.get("accuracy", {}).get("outputs"), file=sys.stderr, flush=True)
    x, y = pow_grid()
    e, ok = pow_errors(oracle_eval(lib, OP["pow"], x, y)[0], x, y)
    i = int(np.argmax(e))
    doc["pow"] = {"measure": "ulp", "worst": repr(float(e[i])), "at": [repr(float(x[i])), repr(float(y[i]))], "pairs_compared": int(ok.sum())}
    ya, xa = atan2_grid()
    e = atan2_errors(oracle_eval(lib, OP["atan2"], ya, xa)[0], ya, xa)
    i = int(np.argmax(e))
    doc["atan2"] = {"measure": "ulp", "worst": repr(float(e[i])), "at": [repr(float(ya[i])), repr(float(xa[i]))], "pairs_compared": int(e.size)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, file=sys.stderr)


if __name__ == "__main__":
    main()
