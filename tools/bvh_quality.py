#!/usr/bin/env python3
"""Quality of the BVH that ppg_set_scene builds, measured on the CPU (no GPU is touched).

Runs the two host-only hooks of include/ppg_testhooks.h — ppg_debug_bvh_stats (node / leaf counts, the surface-area expectation of node
steps and triangle tests on the quantised tree, build time) and ppg_debug_bvh_trace (ordered closest-hit traversal in the kernels' float
arithmetic, counting node steps and triangle tests per ray) — on room_scene, torus_scene, the two real scene files where scratch/*.ppgs
exist (tools/make_scenes.sh), and the triangle soups of tests/test_bvh_quality.py.  The ray set is seeded: camera rays on a jittered grid
plus two generations of cosine-distributed rays from the hit points, the mix a path tracer sends.

    tools/bvh_quality.py --tag this                         prints the table, stores it as block `this` of profiles/bvh_quality.json
    tools/bvh_quality.py --tag parent --lib <parent's .so>  the same builder-independent measurement on another build of the library
    tools/bvh_quality.py --golden tests/golden/bvh_quality_parent.json --lib <parent's .so>    the fixtures' figures for the quality test
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "practical-path-guiding_amd"))

f32 = np.float32
PAD_REL = 2e-6  # ppg_set_scene's box padding, relative to the scene's extent


class Stats(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("depth", C.c_uint32), ("n_binary_nodes", C.c_uint32),
                ("leaf_hist", C.c_uint32 * 9), ("stack_need", C.c_uint32),
                ("sa_interior", C.c_double), ("sa_leaf", C.c_double), ("sa_tris", C.c_double), ("build_seconds", C.c_double)]


def bind(lib_path):
    lib = C.CDLL(lib_path)
    lib.ppg_debug_bvh_stats.restype = C.c_int
    lib.ppg_debug_bvh_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.POINTER(Stats)]
    lib.ppg_debug_bvh_trace.restype = C.c_int
    lib.ppg_debug_bvh_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    return lib


def scene_pad(pos):
    pos = np.asarray(pos, np.float32)
    return float(f32(PAD_REL) * f32(np.max(pos.max(0) - pos.min(0))) + f32(1e-30))


def stats(lib, pos, idx, pad, max_leaf=4):
    pos = np.ascontiguousarray(pos, np.float32)
    idx = np.ascontiguousarray(idx, np.uint32)
    st = Stats()
    rc = lib.ppg_debug_bvh_stats(pos.ctypes.data, idx.ctypes.data, idx.shape[0], float(pad), max_leaf, C.byref(st))
    assert rc == 0
    return dict(triangles=int(idx.shape[0]), nodes=st.n_nodes, leaves=st.n_leaves, depth=st.depth, stack_need=st.stack_need, binary_nodes=st.n_binary_nodes,
                leaf_hist=list(st.leaf_hist), sa_interior=st.sa_interior, sa_leaf=st.sa_leaf, sa_tris=st.sa_tris,
                expected_node_steps=1.0 + st.sa_interior, build_seconds=st.build_seconds)


def trace(lib, pos, idx, pad, max_leaf, rays):
    """rays [R, 8] = (o, mint, d, maxt) -> t [R], original index [R] (-1: none), node steps [R], triangle tests [R], deepest stack"""
    pos = np.ascontiguousarray(pos, np.float32)
    idx = np.ascontiguousarray(idx, np.uint32)
    rays = np.ascontiguousarray(rays, np.float32)
    n = rays.shape[0]
    t, orig = np.empty(n, np.float32), np.empty(n, np.int32)
    steps, tests = np.empty(n, np.uint32), np.empty(n, np.uint32)
    deepest = C.c_uint32(0)
    rc = lib.ppg_debug_bvh_trace(pos.ctypes.data, idx.ctypes.data, idx.shape[0], float(pad), max_leaf, rays.ctypes.data, n,
                                 t.ctypes.data, orig.ctypes.data, steps.ctypes.data, tests.ctypes.data, C.addressof(deepest))
    assert rc == 0
    return t, orig, steps, tests, deepest.value


def make_rays(o, d, maxt=np.inf):
    """the kernels' adaptive ray epsilon: mint = 1e-4 * max(|o|_inf, 1e-4)"""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    rays = np.empty((o.shape[0], 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3] = f32(1e-4) * np.maximum(np.abs(o).max(1), f32(1e-4))
    rays[:, 7] = maxt
    return rays


def camera_rays(cam, rng, nx=96, ny=54):
    s2c = np.asarray(cam["sample_to_camera"], np.float64).reshape(4, 4)
    c2w = np.asarray(cam["camera_to_world"], np.float64).reshape(4, 4)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny))
    sx = (gx.ravel() + rng.uniform(size=nx * ny)) / nx
    sy = (gy.ravel() + rng.uniform(size=nx * ny)) / ny
    p = np.stack([sx, sy, np.zeros_like(sx), np.ones_like(sx)], 1) @ s2c.T
    d = p[:, :3] / p[:, 3:4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ c2w[:3, :3].T
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return o.astype(np.float32), d.astype(np.float32)


def cosine_bounce(pos, idx, o, d, t, orig, rng):
    """next generation: from every hit point, a cosine-distributed direction about the geometric normal on the side the ray came from"""
    hit = orig >= 0
    o, d, t, orig = o[hit].astype(np.float64), d[hit].astype(np.float64), t[hit].astype(np.float64), orig[hit]
    v = np.asarray(pos, np.float64)[np.asarray(idx)[orig]]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    o, d, t, n, ln = o[ok], d[ok], t[ok], n[ok], ln[ok]
    n /= ln[:, None]
    n[np.einsum("ij,ij->i", n, d) > 0] *= -1
    p = o + d * t[:, None]
    u1, u2 = rng.uniform(size=p.shape[0]), rng.uniform(size=p.shape[0])
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(n[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    s = np.cross(n, a)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    b = np.cross(n, s)
    w = s * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + n * np.sqrt(np.maximum(0, 1 - u1))[:, None]
    return p.astype(np.float32), w.astype(np.float32)


def measure_scene(lib, desc, seed=7, max_leaf=4):
    """stats + the traced counts over camera rays and two generations of diffuse bounces"""
    pos, idx = np.asarray(desc.positions, np.float32).reshape(-1, 3), np.asarray(desc.indices, np.uint32).reshape(-1, 3)
    pad = scene_pad(pos)
    rng = np.random.default_rng(seed)
    out = stats(lib, pos, idx, pad, max_leaf)
    o, d = camera_rays(desc.camera, rng)
    n_rays = steps_sum = tests_sum = 0
    deepest = 0
    per_gen = []
    for gen in range(3):
        t, orig, steps, tests, deep = trace(lib, pos, idx, pad, max_leaf, make_rays(o, d))
        per_gen.append(dict(rays=int(o.shape[0]), node_steps_per_ray=float(steps.mean()), triangle_tests_per_ray=float(tests.mean())))
        n_rays += o.shape[0]
        steps_sum += int(steps.sum())
        tests_sum += int(tests.sum())
        deepest = max(deepest, deep)
        if gen < 2:
            o, d = cosine_bounce(pos, idx, o, d, t, orig, rng)
    out.update(rays=n_rays, node_steps_per_ray=steps_sum / n_rays, triangle_tests_per_ray=tests_sum / n_rays, deepest_stack=deepest, generations=per_gen)
    return out


# ---- the triangle soups of tests/test_bvh_quality.py ----
def soup(rng, n, sigma=0.15):
    c = rng.uniform(-1, 1, (n, 3))
    v = (c[:, None, :] + rng.normal(0, sigma, (n, 3, 3))).astype(np.float32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def shared_centroid(rng, n=600):
    """every triangle's box is centred on the origin: no split plane separates any centroids"""
    e = rng.uniform(0.05, 1.0, (n, 3))
    sgn = rng.choice([-1.0, 1.0], (n, 3))
    v = np.empty((n, 3, 3))
    v[:, 0], v[:, 1] = e * sgn, -e * sgn  # two opposite corners of the box: the centroid of the box is exactly 0
    v[:, 2] = rng.uniform(-1, 1, (n, 3)) * e
    return v.astype(np.float32).reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def slivers(rng, n=800):
    """aspect 1000 : 1, in random directions"""
    c = rng.uniform(-1, 1, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    v = np.stack([c - u, c + u, c + w * 2e-3], 1).astype(np.float32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def floor_and_clutter(rng, n=500):
    """two room-sized triangles (a floor) under n small ones: the large boxes a top-down build drags through every level"""
    p, i = soup(rng, n, sigma=0.03)
    big = np.array([[-1.2, -1.2, -0.5], [1.2, -1.2, -0.5], [1.2, 1.2, -0.5], [-1.2, -1.2, -0.5], [1.2, 1.2, -0.5], [-1.2, 1.2, -0.5]], np.float32)
    pos = np.concatenate([big, p])
    idx = np.concatenate([np.array([[0, 1, 2], [3, 4, 5]], np.uint32), i + 6])
    return pos, idx


def doubled(rng, n=300):
    """every triangle twice: all boxes, centroids and hit distances tie"""
    p, i = soup(rng, n)
    return np.concatenate([p, p]), np.concatenate([i, i + p.shape[0]])


def room_fixture(rng):
    import ppg_host
    d = ppg_host.room_scene(64, 48, n_boxes=30, tess=2)
    return np.asarray(d.positions, np.float32).reshape(-1, 3), np.asarray(d.indices, np.uint32).reshape(-1, 3)


FIXTURES = {
    "soup-5": lambda rng: soup(rng, 5), "soup-9": lambda rng: soup(rng, 9), "soup-65": lambda rng: soup(rng, 65), "soup-1500": lambda rng: soup(rng, 1500),
    "shared-centroid-600": shared_centroid, "slivers-800": slivers, "floor-and-clutter-502": floor_and_clutter, "doubled-600": doubled,
    "room-30-boxes": room_fixture,
}


def fixture(name):
    """(positions, indices, rays): seeded by the name's position in FIXTURES, ~300 rays from surface points and from outside"""
    rng = np.random.default_rng(4000 + list(FIXTURES).index(name))
    pos, idx = FIXTURES[name](rng)
    n, R = idx.shape[0], 300
    ext = float(np.max(pos.max(0) - pos.min(0)))
    centre = pos.mean(0)
    o = np.empty((R, 3), np.float32)
    d = rng.normal(size=(R, 3))
    o[: R // 2] = pos[idx[rng.integers(0, n, R // 2)]].mean(1)
    o[R // 2:] = centre + rng.normal(size=(R - R // 2, 3)) * 2 * ext
    d[R // 2:] = centre - o[R // 2:] + rng.normal(size=(R - R // 2, 3)) * 0.3 * ext
    d[::7, 0] = 0.0
    d[::11, 1] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pos, idx, make_rays(o, d.astype(np.float32))


def measure_fixture(lib, name, max_leaf=4):
    pos, idx, rays = fixture(name)
    pad = scene_pad(pos)
    out = stats(lib, pos, idx, pad, max_leaf)
    _, _, steps, tests, deep = trace(lib, pos, idx, pad, max_leaf, rays)
    out.update(rays=int(rays.shape[0]), node_steps_per_ray=float(steps.mean()), triangle_tests_per_ray=float(tests.mean()), deepest_stack=deep)
    return out


def scenes():
    import ppg_host
    yield "room (bench.py --scene room: 1820 boxes)", lambda: ppg_host.room_scene(1280, 720, n_boxes=1820)
    yield "torus", lambda: ppg_host.torus_scene()
    for name in ("kitchen-improved", "spaceship"):
        path = os.path.join(ROOT, "scratch", name + ".ppgs")
        if os.path.exists(path):
            yield name, (lambda p=path: ppg_host.load_scene_file(p))


def main():
    import ppg_host
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="libppg_hip.so to measure (default: this tree's)")
    ap.add_argument("--tag", default="this", help="block of the output file that receives the table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bvh_quality.json"))
    ap.add_argument("--golden", help="write only the fixtures' figures to this file (the parent's values for tests/test_bvh_quality.py)")
    ap.add_argument("--max-leaf", type=int, default=4)
    ap.add_argument("--fixtures-only", action="store_true")
    args = ap.parse_args()
    lib = bind(args.lib or ppg_host.hip_library_path())
    table = {}
    fmt = "%-44s %9s %8s %6s %9s %9s %9s %9s %6s %8s"
    print(fmt % ("scene", "triangles", "nodes", "depth", "E[steps]", "E[tests]", "steps/ray", "tests/ray", "stack", "build s"))

    def show(name, r):
        print(fmt % (name, r["triangles"], r["nodes"], r["depth"], "%.3f" % r["expected_node_steps"], "%.3f" % r["sa_tris"],
                     "%.3f" % r["node_steps_per_ray"], "%.3f" % r["triangle_tests_per_ray"], r["deepest_stack"], "%.3f" % r["build_seconds"]), flush=True)

    if not args.golden and not args.fixtures_only:
        for name, make in scenes():
            table[name] = measure_scene(lib, make(), max_leaf=args.max_leaf)
            show(name, table[name])
    for name in FIXTURES:
        table[name] = measure_fixture(lib, name, args.max_leaf)
        show(name, table[name])
    if args.golden:
        keep = ("triangles", "rays", "node_steps_per_ray", "triangle_tests_per_ray", "expected_node_steps", "sa_tris")
        with open(args.golden, "w") as f:
            json.dump({"produced_by": "tools/bvh_quality.py --golden, run on the library of the commit BEFORE the re-optimising builder (binned SAH, greedy collapse)",
                       "margin_relative": 0.0005,
                       "margin_note": "tests/test_bvh_quality.py asks for values below parent * (1 - margin_relative).  The reductions measured with the new "
                                      "builder are 0.25 % (doubled-600: a random soup, where no builder has structure to find) to 20 % (shared-centroid-600) "
                                      "in traced node steps per ray; the margin is a fifth of the smallest.",
                       "max_leaf": args.max_leaf, "fixtures": {n: {k: table[n][k] for k in keep} for n in FIXTURES}}, f, indent=1)
        return
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.setdefault("cpu_table", {})[args.tag] = table
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
