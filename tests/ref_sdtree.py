"""ctypes side of oracle/ref_sdtree/harness.cpp: the reference's own SD-tree classes (guided_path.cpp up to its integrator class), compiled
by build() into oracle/_ref/libppg_ref_sdtree.so under strict IEEE float evaluation.  Trees travel in the layout of Engine.read_sdtree()."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libppg_ref_sdtree.so")
REFERENCE = os.environ.get("PPG_REFERENCE_DIR", "/root/reference")
REFERENCE_SRC = os.path.join(REFERENCE, "mitsuba", "src", "integrators", "path", "guided_path.cpp")
SKIP_REASON = "needs oracle/_ref/libppg_ref_sdtree.so (built by build() where the reference checkout exists) or the reference checkout itself"

DELTA = np.float32(2.0 ** -23)  # 4e-7 (atan2 bound of test_detmath.py) / 2 pi = 6.4e-8, rounded up to one float ulp at 1.0
SINCOS_TOL = 1.5e-7 + 2 * 2.0 ** -23  # sincos bound of test_detmath.py + 1 ulp for libm + 1 ulp for sqrt(1 - cos^2)


def reference_available():
    """Without side effects (safe at collection time): the library is there, or can be made from the reference checkout."""
    return os.path.exists(REF_SO) or bool(os.path.isfile(REFERENCE_SRC) and shutil.which("g++") and shutil.which("make"))


_built = []


def ensure_built():
    """Once per process: where the reference checkout exists, `make` (incremental, so a library older than harness.cpp is refreshed);
    elsewhere the library that travelled with the tree is used as it is."""
    if not _built:
        if os.path.isfile(REFERENCE_SRC) and shutil.which("g++") and shutil.which("make"):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref_sdtree"), "REFERENCE=" + REFERENCE])
        _built.append(os.path.exists(REF_SO))
    return _built[0]


def second_opinion():
    """A Ref for the tests that merely add the reference's answer to their own; None, with a warning, where it cannot be had."""
    if reference_available() and ensure_built():
        return Ref()
    import warnings
    warnings.warn("oracle/_ref/libppg_ref_sdtree.so is absent and cannot be built here: the reference's second opinion was NOT taken")
    return None


class DTrees(C.Structure):
    _fields_ = [("offset", C.c_void_p), ("num_nodes", C.c_void_p), ("max_depth", C.c_void_p), ("sum", C.c_void_p),
                ("stat_weight", C.c_void_p), ("node_sums", C.c_void_p), ("node_children", C.c_void_p)]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class Ref:
    """The harness holds one STree at a time (loaded from arrays)."""

    def __init__(self):
        assert ensure_built(), SKIP_REASON
        self.lib = C.CDLL(REF_SO)
        self._keep = []

    def _dtrees(self, d):
        arrs = [np.ascontiguousarray(d["offset"], np.uint64), np.ascontiguousarray(d["num_nodes"], np.uint32),
                np.ascontiguousarray(d["max_depth"], np.int32), _f32(d["sum"]), _f32(d["stat_weight"]),
                _f32(d["node_sums"]), np.ascontiguousarray(d["node_children"], np.uint16)]
        self._keep += arrs
        return DTrees(*[a.ctypes.data for a in arrs])

    def load(self, tree, sampling=True, building=True, adam=None):
        """tree: Engine.read_sdtree().  adam: [n][6] uint32 words, or None for (theta of the tree, everything else zero)."""
        self._keep = []
        n = len(tree["axis"])
        if adam is None:
            adam = np.zeros((n, 6), np.uint32)
            adam[:, 0] = _f32(tree["theta"]).view(np.uint32)
        adam = np.ascontiguousarray(adam, np.uint32)
        axis = np.ascontiguousarray(tree["axis"], np.int32)
        ch = np.ascontiguousarray(tree["children"], np.uint32)
        lo, hi = _f32(tree["aabb_min"]), _f32(tree["aabb_max"])
        s = self._dtrees(tree["sampling"]) if sampling else None
        b = self._dtrees(tree["building"]) if building else None
        rc = self.lib.ppgr_stree_load(_ptr(lo), _ptr(hi), C.c_uint32(n), _ptr(axis), _ptr(ch), C.byref(s) if s else None,
                                      C.byref(b) if b else None, _ptr(adam))
        assert rc == 0

    def read(self):
        n, nl, ns, nb = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        assert self.lib.ppgr_info(C.byref(n), C.byref(nl), C.byref(ns), C.byref(nb)) == 0
        n = n.value
        axis, ch = np.zeros(n, np.int32), np.zeros((n, 2), np.uint32)
        assert self.lib.ppgr_read_stree(_ptr(axis), _ptr(ch)) == 0
        out = {"axis": axis, "children": ch, "n_leaves": nl.value}
        for which, name, total in ((0, "sampling", ns.value), (1, "building", nb.value)):
            off, nn, md = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.int32)
            sm, sw, mean = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
            sums, nch = np.zeros((total, 4), np.float32), np.zeros((total, 4), np.uint16)
            assert self.lib.ppgr_read_dtrees(which, _ptr(off), _ptr(nn), _ptr(md), _ptr(sm), _ptr(sw), _ptr(mean), _ptr(sums), _ptr(nch)) == 0
            out[name] = {"offset": off, "num_nodes": nn, "max_depth": md, "sum": sm, "stat_weight": sw, "mean": mean,
                         "node_sums": sums, "node_children": nch}
        st = np.zeros((n, 6), np.uint32)
        assert self.lib.ppgr_read_adam(_ptr(st)) == 0
        out["adam"] = st
        out["theta"] = st[:, 0].copy().view(np.float32)
        return out

    def pdf(self, pos, dirs):
        pos, dirs = _f32(pos), _f32(dirs)
        out = np.zeros(len(pos), np.float32)
        assert self.lib.ppgr_pdf(C.c_uint32(len(pos)), _ptr(pos), _ptr(dirs), _ptr(out)) == 0
        return out

    def pdf_canonical(self, pos, xy):
        """(sampling.pdf(xy), sampling.depthAt(xy), S-tree node) of the leaf that holds pos"""
        pos, xy = _f32(pos), _f32(xy)
        out, dep, node = np.zeros(len(pos), np.float32), np.zeros(len(pos), np.int32), np.zeros(len(pos), np.uint32)
        assert self.lib.ppgr_pdf_canonical(C.c_uint32(len(pos)), _ptr(pos), _ptr(xy), _ptr(out), _ptr(dep), _ptr(node)) == 0
        return out, dep, node

    def dir_to_canonical(self, dirs):
        dirs = _f32(dirs)
        xy = np.zeros((len(dirs), 2), np.float32)
        self.lib.ppgr_dir_to_canonical.restype = None
        self.lib.ppgr_dir_to_canonical(C.c_uint32(len(dirs)), _ptr(dirs), _ptr(xy))
        return xy

    def canonical_to_dir(self, xy):
        xy = _f32(xy)
        d = np.zeros((len(xy), 3), np.float32)
        self.lib.ppgr_canonical_to_dir.restype = None
        self.lib.ppgr_canonical_to_dir(C.c_uint32(len(xy)), _ptr(xy), _ptr(d))
        return d

    def sample(self, pos, seed):
        pos = _f32(pos)
        d, c, dims = np.zeros((len(pos), 3), np.float32), np.zeros((len(pos), 2), np.float32), np.zeros(len(pos), np.uint32)
        assert self.lib.ppgr_sample(C.c_uint32(len(pos)), _ptr(pos), C.c_uint64(seed), _ptr(d), _ptr(c), _ptr(dims)) == 0
        return d, c, dims

    def stream(self, seed, n, dim):
        out = np.zeros(n, np.float32)
        self.lib.ppgr_stream.restype = None
        self.lib.ppgr_stream(C.c_uint64(seed), C.c_uint32(n), C.c_uint32(dim), _ptr(out))
        return out

    def build(self):
        assert self.lib.ppgr_build() == 0

    def refine_reset(self, s_tree_threshold, max_mb, max_depth, d_tree_threshold):
        assert self.lib.ppgr_refine_reset(C.c_uint64(int(s_tree_threshold)), C.c_int32(max_mb), C.c_int32(max_depth), C.c_float(d_tree_threshold)) == 0

    def adam_replay(self, state, records, loss):
        """state: 6 uint32 words (theta, iter, m, v, batchGradient, batchAccumulation); records [n][5] float32; loss 1 = kl, 2 = var"""
        state = np.ascontiguousarray(state, np.uint32)
        records = _f32(records).reshape(-1, 5)
        out = np.zeros(6, np.uint32)
        assert self.lib.ppgr_adam_replay(_ptr(state), C.c_uint32(len(records)), _ptr(records), C.c_int32(loss), _ptr(out)) == 0
        return out

    def log_calls(self):
        return self.lib.ppgr_log_calls()


def exercise(fn, acc, dfilter, xy, irr, w, q, seed=5, rho=0.01):
    """ppgo_dtree_exercise / ppgr_dtree_exercise (same signature)"""
    n, m = len(irr), len(q)
    xy, irr, w, q = _f32(xy), _f32(irr), _f32(w), _f32(q)
    pdf, smp = np.zeros(m, np.float32), np.zeros((m, 2), np.float32)
    nn, sums, ch = C.c_uint32(), np.zeros((65536, 4), np.float32), np.zeros((65536, 4), np.uint16)
    sw, ts = C.c_float(), C.c_float()
    rc = fn(C.c_int32(acc), C.c_int32(dfilter), C.c_float(rho), C.c_uint32(n), _ptr(xy), _ptr(irr), _ptr(w), C.c_uint32(m), _ptr(q),
            C.c_uint64(seed), _ptr(pdf), _ptr(smp), C.byref(nn), _ptr(sums), _ptr(ch), C.byref(sw), C.byref(ts))
    assert rc == 0
    return dict(pdf=pdf, samples=smp, n=nn.value, sums=sums[:nn.value].copy(), children=ch[:nn.value].copy(), statw=sw.value, total=ts.value)


def ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.spacing(np.maximum(x, np.float32(1.1754944e-38))).astype(np.float64)
