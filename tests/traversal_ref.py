"""What tests/test_traversal.py (CPU) and tests/test_traversal_gpu.py share: the scenes, the ray classes and a numpy restatement of the
triangle test that can be evaluated in float32 and in float64.  Not a test module.

The restatement is TriAccel::load / TriAccel::rayIntersect (triaccel.h) in the order of operations of csrc/ppg_device.h tri_hit_regs and
csrc/ppg_hip.hip triAccelLoad, over ALL triangles (no tree): closest hit by (t, original index).  In float32 it is what the host walker
and the kernels must return bit for bit; in float64 — records built in float64 from the float32 vertices — it is the reference that is
not the project's float code.

The float64 comparison needs a bound and a notion of rays that no float32 code can be held to:
  figure(rays)   the largest difference between the two evaluations on rays where both find the same triangle — of t relative to t, and
                 of the barycentrics u, v absolutely — the float32 error of this operation at this scene's and these rays' scale.
  bound          8 x figure, this project's usual margin over a measured float32 error.  The figure is taken per ray CLASS (never larger
                 than the figure of the whole scene, which is their maximum): a ray from 1e4 scene extents away loses four digits of
                 its hit point to cancellation and would otherwise set the bound of every other ray of the scene.
  unsure         a ray is left out where float64 itself is within the bound of a decision: the winning triangle's barycentrics or its
                 t against [mint, maxt] are within the bound of the limit, or a triangle that float64 rejects within the bound could win
                 (its t is smaller than the winner's by more than half the bound; a candidate within half the bound of the winner is a
                 tie: either triangle is accepted, and the returned t stays within the bound whichever is taken).
"""
import os
import sys

import numpy as np

from conftest import ROOT
from test_bvh_host import EMPTY, scale_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_quality as bq  # noqa: E402

f32 = np.float32
EPS = f32(1e-4)  # PPG_EPSILON


# ---------------------------------------------------------------------------------------------------------------- scenes
def nested_soup(n, r):
    """n nested triangles (s, -s, -s) (s, s, -s) (s, 0, s), s = r**k: the SAH sweep peels one per level"""
    s = np.float64(r) ** np.arange(n)
    z = np.zeros_like(s)
    v = np.stack([np.stack([s, -s, -s], 1), np.stack([s, s, -s], 1), np.stack([s, z, s], 1)], 1).astype(np.float32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


NESTED = [(n, r) for n in (60, 120, 400) for r in (0.5, 0.7, 0.8)]
LARGEST_NESTED = (400, 0.8)


def nested_rays(n, r):
    """along +x from the origin through every triangle (the deep walk), and a fan about it"""
    rng = np.random.default_rng(int(n * 10 + r * 10))
    d = np.concatenate([[[1.0, 0.0, 0.0]], np.concatenate([np.ones((63, 1)), rng.normal(0, 0.2, (63, 2))], 1)])
    o = np.zeros_like(d)
    o[32:] = [-0.5, 0.0, 0.0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return bq.make_rays(o, d.astype(np.float32))


def pos_idx(desc):
    return np.asarray(desc.positions, np.float32).reshape(-1, 3), np.asarray(desc.indices, np.uint32).reshape(-1, 3)


def doubled_room(n_boxes=50, tess=2):
    """room_scene with every box twice, the copy's triangles in reverse order (test_gpu_parity's coincident-triangle scene)"""
    import ppg_host
    scene = ppg_host.room_scene(96, 54, n_boxes=n_boxes, tess=tess, glossy=True)
    idx, mat, em = np.asarray(scene.indices).reshape(-1, 3), np.asarray(scene.tri_material), np.asarray(scene.tri_emitter)
    boxes = np.arange(24, len(idx))
    scene.indices = np.concatenate([idx, idx[boxes][::-1]]).astype(idx.dtype)
    scene.tri_material = np.concatenate([mat, mat[boxes][::-1]])
    scene.tri_emitter = np.concatenate([em, em[boxes][::-1]])
    return scene


def coincident_fan(n=600, seed=5, distinct=6):
    """n triangles that are `distinct` large overlapping ones about one centre, each n / distinct times: every hit is a tie across many
    leaves, no box of a copy is culled by the hit on another (its entry distance is not beyond the hit), and a ray that hits walks
    every copy — more entries than one row of the wave-wide stack holds"""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 1.0, (distinct, 3, 3)) + rng.normal(0, 0.05, (distinct, 1, 3))
    v = base[np.arange(n) % distinct]
    return v.astype(np.float32).reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def desc_of(pos, idx, normals=None):
    """a diffuse scene description of a triangle soup (one emitter: the first triangle), seen from outside"""
    import ppg_host
    n = idx.shape[0]
    emitter = np.full(n, -1, np.int32)
    emitter[0] = 0
    material = (np.arange(n) % 3).astype(np.uint32)
    mats = [dict(type=0, reflectance=(0.7, 0.6, 0.5)), dict(type=0, reflectance=(0.2, 0.6, 0.5)), dict(type=0, reflectance=(0.7, 0.1, 0.5))]
    cam = ppg_host.scenes.perspective_camera((0.3, -3.2, 1.1), (0.0, 0.0, -0.1), (0, 0, 1), 45.0, "x", 0.01, 100.0, 32, 24)
    return ppg_host.SceneDesc(pos, idx, material, emitter, mats, [dict(radiance=(12.0, 12.0, 12.0))], cam, normals=normals)


# ---------------------------------------------------------------------------------------------------------------- the triangle test
def triaccel(pos, idx, dtype):
    """TriAccel::load for all triangles in `dtype` (float32: triAccelLoad operation for operation)"""
    P = pos.astype(np.float32).astype(dtype)
    A, B, Cc = (P[idx[:, k]] for k in range(3))
    b, c = Cc - A, B - A
    N = np.stack([c[:, 1] * b[:, 2] - c[:, 2] * b[:, 1], c[:, 2] * b[:, 0] - c[:, 0] * b[:, 2], c[:, 0] * b[:, 1] - c[:, 1] * b[:, 0]], 1)
    kk = np.argmax(np.abs(N), axis=1)  # the first of equal maxima, like the strict > of the loop
    u, v = (kk + 1) % 3, (kk + 2) % 3
    r = np.arange(idx.shape[0])
    n_k = N[r, kk]
    denom = b[r, u] * c[r, v] - b[r, v] * c[r, u]
    with np.errstate(all="ignore"):
        rec = dict(n_u=N[r, u] / n_k, n_v=N[r, v] / n_k, n_d=((A[:, 0] * N[:, 0] + A[:, 1] * N[:, 1]) + A[:, 2] * N[:, 2]) / n_k,
                   a_u=A[r, u], a_v=A[r, v], b_nu=b[r, u] / denom, b_nv=-b[r, v] / denom, c_nu=c[r, v] / denom, c_nv=-c[r, u] / denom)
    assert all(x.dtype == dtype for x in rec.values())
    rec.update(k=np.where(denom == 0, 3, kk), u=u, v=v)
    return rec


def tri_tuv(rec, rays, dtype, chunk=128):
    """TriAccel::rayIntersect's t, u, v of every (ray, triangle) in `dtype` -> three [R, T] arrays (degenerate triangles: NaN)"""
    R, T = rays.shape[0], rec["k"].shape[0]
    t_all, u_all, v_all = (np.empty((R, T), dtype) for _ in range(3))
    ok = rec["k"] < 3
    ku, kv, kk = rec["u"], rec["v"], np.minimum(rec["k"], 2)
    with np.errstate(all="ignore"):
        for s in range(0, R, chunk):
            o, d = rays[s:s + chunk, 0:3].astype(dtype), rays[s:s + chunk, 4:7].astype(dtype)
            o_u, o_v, o_k = o[:, ku], o[:, kv], o[:, kk]
            d_u, d_v, d_k = d[:, ku], d[:, kv], d[:, kk]
            t = (((rec["n_d"] - o_u * rec["n_u"]) - o_v * rec["n_v"]) - o_k) / ((d_u * rec["n_u"] + d_v * rec["n_v"]) + d_k)
            hu = (o_u + t * d_u) - rec["a_u"]
            hv = (o_v + t * d_v) - rec["a_v"]
            uu = hv * rec["b_nu"] + hu * rec["b_nv"]
            vv = hu * rec["c_nu"] + hv * rec["c_nv"]
            assert t.dtype == dtype and uu.dtype == dtype
            t[:, ~ok] = np.nan
            t_all[s:s + chunk], u_all[s:s + chunk], v_all[s:s + chunk] = t, uu, vv
    return t_all, u_all, v_all


def closest(t, u, v, rays, dtype):
    """closest hit by (t, original index) of tri_tuv's arrays -> t [R] (inf: none), index [R] (-1)"""
    mint, maxt = rays[:, 3].astype(dtype)[:, None], rays[:, 7].astype(dtype)[:, None]
    with np.errstate(all="ignore"):
        hit = ~(t < mint) & ~(t > maxt) & (u >= 0) & (v >= 0) & (u + v <= dtype(1.0)) & ~np.isnan(t)
    tt = np.where(hit, t, np.inf)
    best = np.argmin(tt, axis=1)  # the first of equal minima: the smallest original index
    r = np.arange(t.shape[0])
    found = hit[r, best]
    return np.where(found, tt[r, best], np.inf).astype(dtype), np.where(found, best, -1).astype(np.int32)


def brute32(pos, idx, rays):
    t, u, v = tri_tuv(triaccel(pos, idx, np.float32), rays, np.float32)
    return closest(t, u, v, rays, np.float32)


RESOLVE = 0.1
EXACT_ONLY = ("at-edges", "at-vertices", "maxt-equals-t", "maxt-just-below-t", "mint-equals-t", "mint-just-above-t")


class Reference64:
    """the float64 closest hit of `rays`, the float32-float64 figure per ray class, and which rays are unsure"""

    def __init__(self, pos, idx, rays, classes):
        self.rays, self.classes = rays, classes
        t32, u32, v32 = tri_tuv(triaccel(pos, idx, np.float32), rays, np.float32)
        self.t32, self.i32 = closest(t32, u32, v32, rays, np.float32)
        t, u, v = tri_tuv(triaccel(pos, idx, np.float64), rays, np.float64)
        self.t_all = t
        self.t, self.i = closest(t, u, v, rays, np.float64)
        r = np.arange(rays.shape[0])
        both = (self.i >= 0) & (self.i == self.i32)
        w = np.maximum(self.i, 0)
        with np.errstate(all="ignore"):
            rel_t = np.abs(self.t32.astype(np.float64) - self.t) / np.abs(self.t)
            duv = np.maximum(np.abs(u32[r, w].astype(np.float64) - u[r, w]), np.abs(v32[r, w].astype(np.float64) - v[r, w]))
        per_ray = np.where(both, np.maximum(rel_t, duv), 0.0)
        self.uv = np.stack([u[r, w], v[r, w]], 1)  # of the float64 winner, in float64 and as the float32 evaluation has them
        self.uv32 = np.stack([u32[r, w], v32[r, w]], 1)
        # the figure of a class, and the bound of every ray: 8 x its class's figure (floor: the rounding of one float32 operation)
        self.figure = {}
        self.bound = np.zeros(rays.shape[0])
        for name, sl in classes.items():
            self.figure[name] = float(per_ray[sl].max()) if per_ray[sl].size else 0.0
            self.bound[sl] = 8.0 * max(self.figure[name], 2.0 ** -24)
        B = self.bound[:, None]
        mint, maxt = rays[:, 3].astype(np.float64)[:, None], rays[:, 7].astype(np.float64)[:, None]
        with np.errstate(all="ignore"):
            bt = B * np.abs(t)
            maybe = (t >= mint - bt) & (t <= maxt + bt) & (u >= -B) & (v >= -B) & (u + v <= 1 + B)
            firm = (t >= mint + bt) & (t <= maxt - bt) & (u >= B) & (v >= B) & (u + v <= 1 - B)
        self.maybe = maybe
        tw = np.where(self.i >= 0, self.t, np.inf)[:, None]
        btw = (self.bound * np.abs(np.where(self.i >= 0, self.t, 0.0)))[:, None]
        earlier = (maybe & (t < tw - 0.5 * btw)).any(1)  # (a strict float64 hit is never earlier than the winner: these are near misses)
        winner_firm = np.where(self.i >= 0, firm[r, w], True)
        self.unsure = earlier | ~winner_firm
        with np.errstate(all="ignore"):
            self.tie = maybe & (np.abs(t - tw) <= 0.5 * btw)  # [R, T]: the triangles a sure ray may report
        # the classes that sit ON a decision by construction — a t-window that ends at the hit, a ray aimed at an edge or a vertex — are
        # held exactly (kernels = host walker = float32 all-triangles closest hit) and have no float64 statement to make
        # ... nor has a class whose bound exceeds RESOLVE of a triangle: float32 cannot tell the triangles apart at that scale (triangles
        # of a hundredth of the scene seen from 1e4 scene extents away; the dust at the centre of the nested soup).  Decided by the two
        # numpy evaluations alone, never by the code under test.
        self.exact_only = set(EXACT_ONLY) | {name for name in classes if 8.0 * self.figure[name] > RESOLVE}
        self.scene_figure = max(self.figure[name] for name in classes if name not in self.exact_only)  # of what is compared
        self.applies = np.ones(rays.shape[0], bool)
        for name in self.exact_only:
            if name in classes:
                self.applies[classes[name]] = False

    def check(self, t_dev, orig_dev):
        """asserts of the float64 comparison on the sure rays; returns how many were compared"""
        sure = ~self.unsure & self.applies
        hit = self.i >= 0
        assert np.array_equal(orig_dev[sure] >= 0, hit[sure]), np.nonzero(sure & ((orig_dev >= 0) != hit))[0][:8]
        s = np.nonzero(sure & hit)[0]
        assert self.tie[s, orig_dev[s]].all(), s[~self.tie[s, orig_dev[s]]][:8]
        err = np.abs(t_dev[s].astype(np.float64) - self.t[s])
        lim = self.bound[s] * np.abs(self.t[s])
        assert (err <= lim).all(), (s[err > lim][:8], err[err > lim][:8], lim[err > lim][:8])
        return int(sure.sum())

    def counted(self):
        """per class the float64 comparison applies to: rays that are sure"""
        return {name: int((~self.unsure[sl]).sum()) for name, sl in self.classes.items() if name not in self.exact_only}

    def unsure_fraction(self):
        return float(self.unsure[self.applies].mean())


# ---------------------------------------------------------------------------------------------------------------- rays
def box_planes(nodes):
    """the decoded planes of every child box, as the kernels' float decode gives them: [(axis, value), ...]"""
    out = []
    for nd in nodes:
        for a in range(3):
            s = scale_of((int(nd["exps"]) >> (8 * a)) & 255)
            for k in range(4):
                if int(nd["child"][k]) == EMPTY:
                    continue
                for q in (nd["qlo"], nd["qhi"]):
                    out.append((a, f32(nd["org"][a]) + f32((int(q[a]) >> (8 * k)) & 255) * s))
    return out


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _rays(o, d, mint=None, maxt=np.inf):
    rays = bq.make_rays(np.asarray(o, np.float32), np.asarray(d, np.float32), maxt)
    if mint is not None:
        rays[:, 3] = mint
    # k_trace rescales a mint that equals PPG_EPSILON exactly: keep the scaled values off it (include/ppg_testhooks.h KTRACE)
    rays[rays[:, 3] == EPS, 3] = np.nextafter(EPS, f32(1))
    return rays


def ray_classes(lib, pos, idx, nodes, max_leaf, seed, k=64, k_random=512, k_far=96):
    """rays [R, 8] and {class: slice}.  Finite rays only.  The classes that need a first hit take it from the host walker."""
    rng = np.random.default_rng(seed)
    n = idx.shape[0]
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    ext, centre = float((hi - lo).max()), 0.5 * (lo + hi)
    pad = bq.scene_pad(pos)
    tri = pos[idx].astype(np.float64)  # [n, 3, 3]

    def on_triangles(m):
        w = rng.dirichlet([1.0, 1.0, 1.0], m)
        return np.einsum("mk,mkc->mc", w, tri[rng.integers(0, n, m)])

    def outside(m, dist=2.0):
        return centre + _unit(rng.normal(size=(m, 3))) * dist * ext

    parts = {}
    o = outside(k_random)
    parts["random-outside"] = _rays(o, _unit(on_triangles(k_random) - o))
    parts["random-inside"] = _rays(rng.uniform(lo, hi, (k_random, 3)), _unit(rng.normal(size=(k_random, 3))))
    for name, zeros in (("one-zero-component", 1), ("two-zero-components", 2)):
        d = rng.normal(size=(k, 3))
        for j in range(k):
            d[j, rng.permutation(3)[:zeros]] = 0.0
        d = _unit(d)
        # (through a point inside the scene's box — not one of a triangle: in an axis-aligned scene such a ray would run IN a wall's plane)
        parts[name] = _rays(rng.uniform(lo, hi, (k, 3)) - d * rng.uniform(0.2, 1.5, (k, 1)) * ext, d)
    # origins lying exactly in a decoded box plane, the direction's component along that axis zero (the ray runs in the plane) or not
    planes = box_planes(nodes)
    pick = rng.integers(0, len(planes), k)
    o = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (k, 3)).astype(np.float32)
    d = _unit(centre + rng.normal(0, 0.3 * ext, (k, 3)) - o)
    for j in range(k):
        a, val = planes[pick[j]]
        o[j, a] = val
        if j % 2 == 0:
            d[j, a] = 0.0
    parts["in-a-box-plane"] = _rays(o, _unit(d))
    # aimed at shared edges (the midpoint of a triangle's edge) and at vertices, with float32 directions
    which = rng.integers(0, n, k)
    e = rng.integers(0, 3, k)
    o = outside(k)
    parts["at-edges"] = _rays(o, _unit(0.5 * (tri[which, e] + tri[which, (e + 1) % 3]) - o))
    o = outside(k)
    parts["at-vertices"] = _rays(o, _unit(tri[rng.integers(0, n, k), rng.integers(0, 3, k)] - o))
    parts["from-a-triangle"] = _rays(on_triangles(k), _unit(rng.normal(size=(k, 3))))  # (the render's epsilon: make_rays)
    far = centre + _unit(rng.normal(size=(k_far, 3))) * 1e4 * ext
    parts["from-1e4-extents"] = _rays(far, _unit(on_triangles(k_far) - far))
    for name, scale in (("direction-1e-3", 1e-3), ("direction-1e3", 1e3)):
        o = outside(k)
        parts[name] = _rays(o, _unit(on_triangles(k) - o) * scale)
    # the t-window classes: first and second hit of 2 k rays from the host walker
    o = outside(2 * k)
    base = _rays(o, _unit(on_triangles(2 * k) - o))
    t1 = bq.trace(lib, pos, idx, pad, max_leaf, base)[0]
    second = base.copy()
    second[:, 3] = np.nextafter(t1, f32(np.inf))
    t2 = bq.trace(lib, pos, idx, pad, max_leaf, second[np.isfinite(t1)])[0]
    base, t1 = base[np.isfinite(t1)], t1[np.isfinite(t1)]
    assert base.shape[0] >= k  # (the rays are aimed at triangles: they hit)
    base, t1, t2 = base[:k], t1[:k], t2[:k]

    def window(mint=None, maxt=None):
        r = base.copy()
        if mint is not None:
            r[:, 3] = mint
        if maxt is not None:
            r[:, 7] = maxt
        return r
    between = np.where(np.isfinite(t2), t1 + 0.5 * (t2 - t1), t1 * f32(1.5)).astype(np.float32)
    parts["maxt-between-first-and-second"] = window(maxt=between)
    parts["maxt-equals-t"] = window(maxt=t1)
    parts["maxt-just-below-t"] = window(maxt=np.nextafter(t1, f32(0)))
    parts["mint-equals-t"] = window(mint=t1)
    parts["mint-just-above-t"] = window(mint=np.nextafter(t1, f32(np.inf)))
    rays, classes, at = [], {}, 0
    for name, r in parts.items():
        classes[name] = slice(at, at + r.shape[0])
        at += r.shape[0]
        rays.append(r)
    rays = np.concatenate(rays).astype(np.float32)
    assert np.isfinite(rays[:, :7]).all() and not np.isnan(rays[:, 7]).any() and rays.shape[0] <= 4096
    return rays, classes


# ---------------------------------------------------------------------------------------------------------------- fill_isect in float64
def fill_isect_np(pos, idx, normals, orig, u, v, d, dtype):
    """csrc/ppg_device.h fill_isect in `dtype` for hits (original triangle, u, v) of rays with direction d -> p, geo_n, n, s, wi"""
    P = pos.astype(dtype)[idx[orig]]
    u, v, d = u.astype(dtype), v.astype(dtype), d.astype(dtype)
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    b = np.stack([1 - u - v, u, v], 1)
    p = p0 * b[:, :1] + p1 * b[:, 1:2] + p2 * b[:, 2:]
    side1, side2 = p1 - p0, p2 - p0
    fn = np.cross(side1, side2)
    ln = np.linalg.norm(fn, axis=1, keepdims=True)
    fn = np.where(ln > 0, fn / np.where(ln > 0, ln, 1), fn)
    if normals is not None:
        N = normals.astype(dtype)[idx[orig]]
        sh = N[:, 0] * b[:, :1] + N[:, 1] * b[:, 1:2] + N[:, 2] * b[:, 2:]
        sh = sh / np.linalg.norm(sh, axis=1, keepdims=True)
        fn = np.where((np.einsum("ij,ij->i", fn, sh) < 0)[:, None], -fn, fn)
    else:
        sh = fn
    s = side1 - sh * np.einsum("ij,ij->i", sh, side1)[:, None]
    s = s / np.linalg.norm(s, axis=1, keepdims=True)
    t = np.cross(sh, s)
    wi = np.stack([np.einsum("ij,ij->i", -d, s), np.einsum("ij,ij->i", -d, t), np.einsum("ij,ij->i", -d, sh)], 1)
    out = dict(p=p, geo_n=fn, n=sh, s=s, wi=wi)
    assert all(x.dtype == dtype for x in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------- the scenes by name
def with_normals(pos, idx, seed=17):
    """per-vertex normals for a soup of unshared vertices: the geometric normal, tilted, every fourth triangle's flipped against it;
    plus one zero-area triangle (the last)"""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([pos, np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]], np.float32)])
    idx = np.concatenate([idx, np.array([[len(pos) - 3, len(pos) - 2, len(pos) - 1]], np.uint32)])
    assert len(np.unique(idx)) == idx.size  # (no vertex is shared: a normal belongs to one triangle)
    tri = pos[idx].astype(np.float64)
    g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ln = np.linalg.norm(g, axis=1, keepdims=True)
    g = np.where(ln > 0, g / np.where(ln > 0, ln, 1), [[0.0, 0.0, 1.0]])
    g[::4] *= -1
    nrm = np.zeros((len(pos), 3), np.float32)
    for kk in range(3):
        m = g + rng.normal(0, 0.15, g.shape)
        nrm[idx[:, kk]] = (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32)
    return pos, idx, nrm


def grid_soup(seed=3, n=900):
    """small triangles spread evenly: a wide, shallow tree (the top cut of the wave traversal fills its 64 entries)"""
    return bq.soup(np.random.default_rng(seed), n, sigma=0.04)


def cbox_soup():
    import ppg_host
    return pos_idx(ppg_host.cbox_scene(32, 32))


SOUPS = {
    "cbox": cbox_soup,
    "floor-and-clutter-502": lambda: bq.fixture("floor-and-clutter-502")[:2],
    "doubled-600": lambda: bq.fixture("doubled-600")[:2],
    "doubled-room": lambda: pos_idx(doubled_room()),
    "nested-400-0.8": lambda: nested_soup(*LARGEST_NESTED),
    "full-top-cut": grid_soup,
    "coincident-600": coincident_fan,
}
SEEDS = {name: 9100 + k for k, name in enumerate(SOUPS)}
