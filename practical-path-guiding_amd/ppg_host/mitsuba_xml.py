"""Loader for the subset of Mitsuba 0.6 scene XML the reference's bundled scenes use:

  integrator  guided_path (every property of GP:1014-1085 and integrator.cpp:192-218), or a multichannel holding exactly one guided_path
              and any number of field integrators (field, undefined): info["fields"] = [(name, undefined rgb)], the feature buffers
  sensor      perspective (fov, fovAxis or focalLength, nearClip, farClip, toWorld; focusDistance ignored: pinhole),
              thinlens (the same + apertureRadius, focusDistance: SceneDesc.lens; toWorld without scale),
              nested sampler (independent; sampleCount / seed do not steer guided_path, GP:1342-1374) and
              film hdrfilm (width, height; rfilter box / tent / gaussian / mitchell / catmullrom / lanczos)
  shapes      obj (filename, toWorld, faceNormals, maxSmoothAngle, flipNormals, flipTexCoords, collapse),
              serialized (filename, shapeIndex, toWorld, faceNormals, maxSmoothAngle, flipNormals), ply (filename, toWorld, faceNormals, maxSmoothAngle, flipNormals), rectangle / cube (toWorld, flipNormals),
              sphere (center, radius, toWorld = rotation x uniform scale, flipNormals) — analytic, not tessellated,
              disk (toWorld without shear or non-uniform scale, flipNormals), cylinder (p0, p1, radius, toWorld, flipNormals) — analytic
              (SceneDesc.shapes); no textured BSDFs on them; a cylinder must state at least one of p0 / p1 / radius / toWorld
  bsdfs       top level with id, nested in a shape, or <ref id>; one reader per plug-in (_BSDF_READERS):
              diffuse, roughdiffuse (alpha, useFastApprox), difftrans, phong (exponent) — with ensureEnergyConservation,
              conductor (material none, explicit eta / k, or a named material read from Mitsuba's data/ior), plastic, dielectric, thindielectric, null,
              roughconductor / roughdielectric (ggx / beckmann; alpha or alphaU / alphaV, sampleVisible), roughplastic (+ phong; isotropic; reads
              Mitsuba's data/microfacet tables: SceneDesc.rtrans),
              and the adapters, nested as bumpmap | normalmap(mask(twosided(coating | roughcoating | blendbsdf | mixturebsdf(..)))):
              twosided (any of the BRDFs), mask (opacity), coating / roughcoating (intIOR, extIOR, thickness, sigmaA, specularReflectance, alpha;
              constants only; not on dielectrics or the three lobes), blendbsdf (weight) / mixturebsdf (weights) of two / up to four diffuse, conductor,
              roughconductor, plastic or roughplastic children, bumpmap and normalmap (one nested bsdf + one texture with an explicit gamma)
  textures    bitmap (filename, wrapMode[U|V], filterType, gamma, channel, uscale, vscale, uoffset, voffset; .exr / .pfm / .hdr or 8-bit files) and scale
              around one — nested or <ref id> — on reflectance / transmittance / diffuseReflectance, on the specular colours, on the alpha of roughconductor /
              roughdielectric, on a mask's opacity, a blendbsdf's weight and as bump or normal map (SceneDesc.textures); on triangle meshes only
  emitters    point (position or toWorld, intensity), spot (toWorld, intensity, cutoffAngle, beamWidth; no texture), directional (direction or
              toWorld without scale, irradiance): SceneDesc.delta_emitters, samplingWeight 1 only;
              area (nested in a shape), and one environment emitter: constant, envmap (latitude-longitude .exr / .pfm / .hdr; filename, scale, toWorld =
              rotation) or sunsky (baked into an envmap with the tables of a Mitsuba source tree; toWorld = rotation)
  media       homogeneous (sigmaA + sigmaS or sigmaT + albedo, scale, strategy, mediumSamplingWeight) and heterogeneous (method = woodcock; density and
              albedo <volume>s of type constvolume or gridvolume: value, filename of a float32 / uint8 .vol file, toWorld, min / max; scale) with an
              isotropic or hg <phase>, as interior / exterior of a shape or on the sensor, inline or by <ref> (SceneDesc.media)
  values      <spectrum> (value or filename), <rgb>, <srgb>, <blackbody> (spectrum.py), <transform> of translate / rotate / scale / lookAt / matrix,
              <default name value> and $name substitution (mitsuba -D, mitsuba.cpp:58-87)

Anything else raises SceneError naming the plugin (Mitsuba would load it; this path cannot render it yet — SURVEY.md §8(f1)/(f2)).  With
strict=False unsupported BSDFs become diffuse(0.5), adapters that cannot be kept are dropped around their nested BSDF, unsupported emitters and
shapes whose file is missing are skipped, and each such step is listed in `warnings`.

load_scene() is a driver over one reader per element — integrator, sensor and film, named BSDFs, emitters, shapes, assembly — all of them methods
of _Reader, the state of one load.

The OBJ reader follows shapes/obj.cpp:198-342 (fan triangulation of n-gons, negative indices, one mesh per `g` /
`usemtl` run, vertices merged per mesh on identical (position, normal, uv), normals transformed by the inverse
transpose) and TriMesh::computeNormals (trimesh.cpp:608-676: angle-weighted vertex normals when the file has none
and faceNormals is off).  Arithmetic is float32 like the reference's SINGLE_PRECISION build.
"""
import math
import os
import re
import xml.etree.ElementTree as ET

import numpy as np

from . import spectrum
from .bindings import FIELD_NAMES
from .scenes import SceneDesc, perspective_camera_from_matrix

f32 = np.float32
GUIDED_PATH_PROPS = {  # name → type (GP:1014-1085, integrator.cpp:192-218)
    "nee": str, "sampleCombination": str, "spatialFilter": str, "directionalFilter": str, "bsdfSamplingFractionLoss": str,
    "budgetType": str, "sdTreeMaxMemory": int, "sTreeThreshold": int, "dTreeThreshold": float, "bsdfSamplingFraction": float,
    "sppPerPass": int, "budget": float, "dumpSDTree": int, "rrDepth": int, "maxDepth": int, "strictNormals": int, "hideEmitters": int,
}


TEXTURE_KEYS = ("texture", "bump", "normal_map", "specular_texture", "alpha_texture", "opacity_texture", "alpha_v_texture")  # material keys that hold a texture index


class SceneError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------- transforms
def _translate(x, y, z):
    m = np.eye(4, dtype=f32)
    m[:3, 3] = (x, y, z)
    return m


def _scale(x, y, z):
    return np.diag(np.array([x, y, z, 1], f32))


def _mat4_mul(a, b):
    """4x4 product in float64 with a fixed summation order (host/scene_xml.h does the same sums: the two loaders' records are identical)"""
    return np.array([[sum(float(a[i][k]) * float(b[k][j]) for k in range(4)) for j in range(4)] for i in range(4)], np.float64)


def _transform64(elem, sub):
    """A <transform> composed in float64 — every value read as a float, then sums in a fixed order and libm's double sin / cos / sqrt — for
    the analytic disks and cylinders: host/scene_xml.h transform64 does the same operations, so both loaders round the same numbers."""
    m = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for c in elem:
        g = lambda k, d: float(f32(float(sub(c.get(k, str(d))))))  # noqa: E731
        t = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
        if c.tag == "translate":
            t[0][3], t[1][3], t[2][3] = g("x", 0), g("y", 0), g("z", 0)
        elif c.tag == "scale":
            t[0][0], t[1][1], t[2][2] = [g("value", 1)] * 3 if c.get("value") is not None else (g("x", 1), g("y", 1), g("z", 1))
        elif c.tag == "rotate":  # Transform::rotate, transform.cpp:65-97
            ax = (g("x", 0), g("y", 0), g("z", 0))
            ln = math.sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2])
            x, y, z = ax[0] / ln, ax[1] / ln, ax[2] / ln
            th = g("angle", 0) * (math.pi / 180.0)
            s, co = math.sin(th), math.cos(th)
            t[0][:3] = [x * x + (1 - x * x) * co, x * y * (1 - co) - z * s, x * z * (1 - co) + y * s]
            t[1][:3] = [x * y * (1 - co) + z * s, y * y + (1 - y * y) * co, y * z * (1 - co) - x * s]
            t[2][:3] = [x * z * (1 - co) - y * s, y * z * (1 - co) + x * s, z * z + (1 - z * z) * co]
        elif c.tag == "matrix":
            v = _floats(sub(c.get("value")))
            if len(v) != 16:
                raise SceneError("<matrix> needs 16 values")
            t = [[float(f32(v[4 * i + j])) for j in range(4)] for i in range(4)]
        elif c.tag == "lookAt" or c.tag == "lookat":  # Transform::lookAt, transform.cpp:191-214
            o, tg = ([float(f32(v)) for v in _floats(sub(c.get(k)))] for k in ("origin", "target"))
            if len(o) != 3 or len(tg) != 3:
                raise SceneError("<lookAt> needs origin and target")
            cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
            unit = lambda a: [v / math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) for v in a]  # noqa: E731
            d = unit([tg[i] - o[i] for i in range(3)])
            if c.get("up"):
                up = [float(f32(v)) for v in _floats(sub(c.get("up")))]
            else:  # scenehandler.cpp: any vector orthogonal to the viewing direction
                up = cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < abs(d[1]) else [0.0, 1.0, 0.0])
            left = unit(cross(up, d))
            nu = cross(d, left)
            for i in range(3):
                t[i][0], t[i][1], t[i][2], t[i][3] = left[i], nu[i], d[i], o[i]
        else:
            raise SceneError("unsupported transform element <%s>" % c.tag)
        m = _mat4_mul(t, m)  # later elements are applied after earlier ones
    return np.asarray(m, np.float64)


def _linear_part_checks(m, what):
    """Disk::configure's two checks (disk.cpp:105-112) on the first two columns of a 4x4; returns the columns' lengths"""
    c0, c1 = [float(m[a][0]) for a in range(3)], [float(m[a][1]) for a in range(3)]
    l0, l1 = math.sqrt(sum(v * v for v in c0)), math.sqrt(sum(v * v for v in c1))
    if l0 == 0 or l1 == 0:
        raise SceneError("%s: 'toWorld' transformation is singular" % what)
    if abs(sum(a * b for a, b in zip(c0, c1)) / (l0 * l1)) > 1e-3:
        raise SceneError("%s: 'toWorld' transformation contains shear!" % what)
    if abs(l0 / l1 - 1) > 1e-3:
        raise SceneError("%s: 'toWorld' transformation contains a non-uniform scale!" % what)
    return l0, l1


def disk_shape(m, flip_normals):
    """Disk::Disk / configure (disk.cpp:83-115): the record of a <shape type="disk"> under the 4x4 toWorld `m` (SceneDesc.shapes)"""
    l0, l1 = _linear_part_checks(m, "disk")
    l2 = math.sqrt(sum(float(m[a][2]) ** 2 for a in range(3)))
    if not abs(float(np.linalg.det(np.asarray(m, np.float64)[:3, :3]))) > 1e-9 * l0 * l1 * l2:
        raise SceneError("disk: 'toWorld' transformation is singular")
    return dict(type="disk", to_world=[float(f32(m[a][b])) for a in range(3) for b in range(4)], flip_normals=bool(flip_normals))


def cylinder_shape(m, p0, p1, radius, flip_normals):
    """Cylinder::Cylinder (cylinder.cpp:82-108): translate(p0) * fromFrame(Frame(d / |d|)) * scale(r, r, |d|), then toWorld `m` (None: none),
    then the scale moved out of the transform into radius and length.  Float64 sums rounded once (the reference rounds every step to float:
    the records agree to float rounding)."""
    p0, p1 = [float(f32(v)) for v in p0], [float(f32(v)) for v in p1]
    d = [b - a for a, b in zip(p0, p1)]
    length = math.sqrt(sum(v * v for v in d))
    if length == 0:
        raise SceneError("cylinder: p0 and p1 coincide (its length would be 0)")
    radius = float(f32(radius))
    if not radius > 0:
        raise SceneError("cylinder: radius must be > 0")
    a = [v / length for v in d]
    if abs(a[0]) > abs(a[1]):  # coordinateSystem, util.cpp:592-601: Frame(a) = (s, t, a)
        inv = 1.0 / math.sqrt(a[0] * a[0] + a[2] * a[2])
        t = [a[2] * inv, 0.0, -a[0] * inv]
    else:
        inv = 1.0 / math.sqrt(a[1] * a[1] + a[2] * a[2])
        t = [0.0, a[2] * inv, -a[1] * inv]
    sv = [t[1] * a[2] - t[2] * a[1], t[2] * a[0] - t[0] * a[2], t[0] * a[1] - t[1] * a[0]]  # cross(t, a)
    o2w = [[sv[i] * radius, t[i] * radius, a[i] * length, p0[i]] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]
    if m is not None:
        o2w = _mat4_mul(m, o2w)
    l0, _ = _linear_part_checks(o2w, "cylinder")
    c2 = [float(o2w[i][2]) for i in range(3)]
    l2 = math.sqrt(sum(v * v for v in c2))
    for j in (0, 1):  # the axis must stay perpendicular to the circle: otherwise what is left after the scale is removed is no rotation
        cj = [float(o2w[i][j]) for i in range(3)]
        if l2 == 0 or abs(sum(x * y for x, y in zip(cj, c2)) / (math.sqrt(sum(v * v for v in cj)) * l2)) > 1e-3:
            raise SceneError("cylinder: 'toWorld' transformation contains shear!")
    ir, il = 1.0 / l0, 1.0 / l2
    tw = [float(f32(v)) for i in range(3) for v in (float(o2w[i][0]) * ir, float(o2w[i][1]) * ir, float(o2w[i][2]) * il, float(o2w[i][3]))]
    return dict(type="cylinder", to_world=tw, radius=float(f32(l0)), length=float(f32(l2)), flip_normals=bool(flip_normals))


def _rotate(axis, angle_deg):  # Transform::rotate, transform.cpp:65-97
    a = np.asarray(axis, f32)
    a = a / f32(np.sqrt(np.dot(a, a)))
    th = f32(angle_deg) * f32(math.pi / 180.0)
    s, c = f32(np.sin(th)), f32(np.cos(th))
    x, y, z = a
    one = f32(1)
    m = np.eye(4, dtype=f32)
    m[0, :3] = (x * x + (one - x * x) * c, x * y * (one - c) - z * s, x * z * (one - c) + y * s)
    m[1, :3] = (x * y * (one - c) + z * s, y * y + (one - y * y) * c, y * z * (one - c) - x * s)
    m[2, :3] = (x * z * (one - c) - y * s, y * z * (one - c) + x * s, z * z + (one - z * z) * c)
    return m


def _look_at(origin, target, up):  # Transform::lookAt, transform.cpp:191-214
    p, t, u = (np.asarray(v, f32) for v in (origin, target, up))
    d = t - p
    d = d / f32(np.sqrt(np.dot(d, d)))
    left = np.cross(u, d).astype(f32)
    left = left / f32(np.sqrt(np.dot(left, left)))
    new_up = np.cross(d, left).astype(f32)
    m = np.eye(4, dtype=f32)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, new_up, d, p
    return m


def _floats(text):
    return [float(v) for v in text.replace(",", " ").split()]


def _transform(elem, sub):
    m = np.eye(4, dtype=f32)
    for c in elem:
        g = lambda k, d: float(sub(c.get(k, str(d))))  # noqa: E731
        if c.tag == "translate":
            t = _translate(g("x", 0), g("y", 0), g("z", 0))
        elif c.tag == "scale":
            t = _scale(*([g("value", 1)] * 3)) if c.get("value") is not None else _scale(g("x", 1), g("y", 1), g("z", 1))
        elif c.tag == "rotate":
            t = _rotate((g("x", 0), g("y", 0), g("z", 0)), g("angle", 0))
        elif c.tag == "lookAt" or c.tag == "lookat":
            o, tg = _floats(sub(c.get("origin"))), _floats(sub(c.get("target")))
            up = _floats(sub(c.get("up"))) if c.get("up") else None
            if up is None:  # scenehandler.cpp: any vector orthogonal to the viewing direction
                d = np.asarray(tg) - np.asarray(o)
                up = np.cross(d, (1, 0, 0) if abs(d[0]) < abs(d[1]) else (0, 1, 0))
            t = _look_at(o, tg, up)
        elif c.tag == "matrix":
            v = _floats(sub(c.get("value")))
            if len(v) != 16:
                raise SceneError("<matrix> needs 16 values")
            t = np.asarray(v, f32).reshape(4, 4)
        else:
            raise SceneError("unsupported transform element <%s>" % c.tag)
        m = (t @ m).astype(f32)  # scenehandler.cpp: later elements are applied after earlier ones
    return m


def _xf_points(m, p):
    q = p @ m[:3, :3].T + m[:3, 3]
    w = p @ m[3, :3] + m[3, 3]
    return np.where((w != 1)[:, None], q / w[:, None], q).astype(f32)


def _xf_normals(m, n):
    inv_t = np.linalg.inv(m.astype(np.float64))[:3, :3].T.astype(f32)  # Transform::operator()(Normal): inverse transpose
    return (n @ inv_t.T).astype(f32)


# ---------------------------------------------------------------------------------------------- OBJ
def _fetch_lines(path):
    with open(path, "r", errors="replace") as f:
        pending = ""
        for raw in f:
            line = pending + raw.rstrip(" \t\r\n")
            if line.endswith("\\"):  # obj.cpp:166-188: a trailing backslash continues the line
                pending = line[:-1]
                continue
            pending = ""
            yield line
        if pending:
            yield pending


def _unit_angle(u, v):  # util.h:309-314
    d = np.sum(u * v, 1)
    return np.where(d < 0, f32(math.pi) - f32(2) * np.arcsin(f32(0.5) * np.linalg.norm(v + u, axis=1).astype(f32)),
                    f32(2) * np.arcsin(f32(0.5) * np.linalg.norm(v - u, axis=1).astype(f32))).astype(f32)


def compute_normals(pos, tris, flip=False):
    """TriMesh::computeNormals, smooth branch (trimesh.cpp:631-671): angle-weighted face normals, triangle-major."""
    n = np.zeros_like(pos, dtype=f32)
    p = pos[tris]  # (T, 3, 3)
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    fn = np.cross(a, b).astype(f32)
    ln = np.sqrt(np.sum(fn * fn, 1)).astype(f32)
    ok = ln != 0
    fn[ok] = fn[ok] / ln[ok, None]
    idx, contrib = [], []
    for i in range(3):
        v0, v1, v2 = p[:, i], p[:, (i + 1) % 3], p[:, (i + 2) % 3]
        sa, sb = (v1 - v0).astype(f32), (v2 - v0).astype(f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            ua = sa / np.sqrt(np.sum(sa * sa, 1)).astype(f32)[:, None]
            ub = sb / np.sqrt(np.sum(sb * sb, 1)).astype(f32)[:, None]
            ang = _unit_angle(ua, ub)
        idx.append(tris[:, i]); contrib.append(fn * ang[:, None])
    order = np.stack(idx, 1).reshape(-1)            # triangle-major: (t0 c0, t0 c1, t0 c2, t1 c0, ...)
    vals = np.stack(contrib, 1).reshape(-1, 3)
    keep = np.repeat(ok, 3)                          # degenerate triangles contribute nothing ("break" at i == 0)
    np.add.at(n, order[keep], vals[keep])
    length = np.sqrt(np.sum(n * n, 1)).astype(f32)
    if flip:
        length = -length
    bad = length == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (n / length[:, None]).astype(f32)
    n[bad] = (1, 0, 0)
    return n


def _cosf(x):
    """cosf of the C library (the crease threshold of rebuild_topology must not depend on numpy's float32 cosine)."""
    import ctypes
    import ctypes.util
    global _libm_cos
    try:
        _libm_cos
    except NameError:
        _libm_cos = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm_cos.cosf.restype, _libm_cos.cosf.argtypes = ctypes.c_float, [ctypes.c_float]
    return f32(_libm_cos.cosf(float(f32(x))))


def rebuild_topology(pos, uvs, idx, max_angle):
    """TriMesh::rebuildTopology (trimesh.cpp:468-608): vertices are re-merged on (position, uv) and, around every such vertex, the
    incident triangles are greedily clustered by face normal — a new vertex per cluster of faces whose normals differ by less than
    `max_angle` degrees from the cluster's first face — so that the smooth normals computed afterwards stop at creases.
    Returns (positions, uvs or None, indices); new vertices are numbered in the reference's order (sorted by position, then uv;
    clusters in triangle order)."""
    pos = np.asarray(pos, f32); idx = np.asarray(idx, np.int64)
    dp_thresh = _cosf(f32(max_angle) * f32(math.pi / 180.0))  # std::cos(degToRad(maxAngle))
    v0, v1, v2 = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    n = np.cross(v1 - v0, v2 - v0).astype(f32)
    ln = np.sqrt(np.sum(n * n, 1, dtype=f32), dtype=f32)
    ok = ln > f32(2.93873587705571876e-39)  # RCPOVERFLOW_FLT
    fn = np.zeros_like(n)
    fn[ok] = n[ok] / ln[ok, None]
    # the multimap<Vertex, TopoData>: key order (p.x, p.y, p.z[, uv.x, uv.y]), equal keys in insertion order (triangle, corner)
    groups = {}
    for t in range(len(idx)):
        for j in range(3):
            v = int(idx[t, j])
            key = tuple(float(c) for c in pos[v]) + (tuple(float(c) for c in uvs[v]) if uvs is not None else ())
            groups.setdefault(key, []).append(t)
    new_pos, new_uv = [], []
    new_idx = np.full(idx.shape, -1, np.int64)
    for key in sorted(groups):
        entries = groups[key]
        p = np.asarray(key[:3], f32)
        clustered = [False] * len(entries)
        for a, t1 in enumerate(entries):
            if clustered[a]:
                continue
            n1 = fn[t1]
            vertex = len(new_pos)
            new_pos.append(key[:3])
            if uvs is not None:
                new_uv.append(key[3:])
            for b in range(a, len(entries)):
                if clustered[b]:
                    continue
                n2 = fn[entries[b]]
                if np.array_equal(n1, n2) or f32(f32(n1[0] * n2[0]) + f32(n1[1] * n2[1])) + f32(n1[2] * n2[2]) > dp_thresh:
                    for i in range(3):
                        if np.array_equal(pos[idx[entries[b], i]], p):
                            new_idx[entries[b], i] = vertex
                    clustered[b] = True
    assert (new_idx >= 0).all()
    return (np.asarray(new_pos, f32).reshape(-1, 3), np.asarray(new_uv, f32).reshape(-1, 2) if uvs is not None else None,
            new_idx.astype(np.uint32))


def load_obj(path, to_world=None, face_normals=False, flip_normals=False, flip_tex_coords=True, collapse=False, max_smooth_angle=None):
    """→ list of meshes dict(name, material, positions (V,3), normals (V,3) or None, indices (T,3)) in world space."""
    to_world = np.eye(4, dtype=f32) if to_world is None else to_world
    V, N, UV = [], [], []
    tris, meshes = [], []
    material = ""
    name = os.path.splitext(os.path.basename(path))[0]

    def corner(tok):
        parts = tok.split("/")
        p = int(parts[0])
        uv = int(parts[1]) if len(parts) >= 2 and parts[1] else 0
        n = int(parts[2]) if len(parts) == 3 and parts[2] else 0
        if len(parts) > 3:
            raise SceneError("%s: invalid OBJ face format %r" % (path, tok))
        return p, uv, n

    def flush(mesh_name):
        nonlocal tris
        if not tris:
            return
        pos_w = _xf_points(to_world, np.asarray(V, f32).reshape(-1, 3)) if V else np.zeros((0, 3), f32)
        nrm_w = None
        if N:
            nrm_w = _xf_normals(to_world, np.asarray(N, f32).reshape(-1, 3))
            ln = np.sqrt(np.sum(nrm_w * nrm_w, 1)).astype(f32)
            nz = ln != 0
            nrm_w[nz] = nrm_w[nz] / ln[nz, None]
        uvs = np.asarray(UV, f32).reshape(-1, 2) if UV else np.zeros((0, 2), f32)
        vmap, vp, vn, vuv, idx = {}, [], [], [], []
        has_normals = has_uvs = False
        for t in tris:
            tri = []
            for (p, uv, n) in t:
                if p < 0: p += len(V) + 1
                if n < 0: n += len(N) + 1
                if uv < 0: uv += len(UV) + 1
                if p <= 0 or p > len(V):
                    raise SceneError("%s: vertex index %d out of bounds (max %d)" % (path, p, len(V)))
                if n > len(N) or uv > len(UV):
                    raise SceneError("%s: normal / uv index out of bounds" % path)
                pn = tuple(nrm_w[n - 1]) if n else (0.0, 0.0, 0.0)
                has_normals |= bool(n)
                has_uvs |= bool(uv)
                puv = tuple(uvs[uv - 1]) if uv else (0.0, 0.0)
                key = (tuple(pos_w[p - 1]), pn, puv)
                k = vmap.get(key)
                if k is None:
                    k = vmap[key] = len(vp)
                    vp.append(key[0]); vn.append(pn); vuv.append(puv)
                tri.append(k)
            idx.append(tri)
        pos = np.asarray(vp, f32).reshape(-1, 3)
        idx = np.asarray(idx, np.uint32).reshape(-1, 3)
        normals = np.asarray(vn, f32).reshape(-1, 3) if has_normals else None
        muv = np.asarray(vuv, f32).reshape(-1, 2) if has_uvs else None
        if max_smooth_angle is not None:  # obj.cpp:336-343: the file's normals are discarded, creases found from the dihedral angles
            pos, muv, idx = rebuild_topology(pos, muv, idx, max_smooth_angle)
            normals = None
        normals, idx = _finish_normals(pos, normals, idx, face_normals, flip_normals)
        meshes.append(dict(name=mesh_name, material=material, positions=pos, normals=normals, indices=idx, uvs=muv))
        tris = []

    for line in _fetch_lines(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            V.append([float(v) for v in tok[1:4]])
        elif tok[0] == "vn":
            N.append([float(v) for v in tok[1:4]])
        elif tok[0] == "vt":
            u, v = float(tok[1]), float(tok[2]) if len(tok) > 2 else 0.0
            UV.append([u, 1 - v if flip_tex_coords else v])
        elif tok[0] == "g" and not collapse:
            flush(name)
            name = line[1:].strip()
        elif tok[0] == "usemtl":
            if not collapse:
                flush(name)
            material = line[6:].strip()
        elif tok[0] == "f":
            c = [corner(t) for t in tok[1:]]
            if len(c) < 3:
                raise SceneError("%s: face with fewer than 3 vertices" % path)
            for k in range(1, len(c) - 1):  # n-gons as a fan (obj.cpp:322-334)
                tris.append((c[0], c[k], c[k + 1]))
    flush(name)
    return meshes


def rectangle_mesh(to_world, flip_normals=False):
    """shapes/rectangle.cpp:170-203 (createTriMesh)."""
    m = to_world
    if flip_normals:
        m = (m @ _scale(1, 1, -1)).astype(f32)  # rectangle.cpp:82-83
    pos = _xf_points(m, np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], f32))
    n = _xf_normals(m, np.array([[0, 0, 1]], f32))[0]
    n = (n / f32(np.sqrt(np.dot(n, n)))).astype(f32)
    return dict(name="rectangle", material="", positions=pos, normals=np.repeat(n[None], 4, 0), indices=np.array([[0, 1, 2], [2, 3, 0]], np.uint32))


# ---------------------------------------------------------------------------------------------- scene
def _finish_normals(pos, normals, idx, face_normals, flip_normals):
    """TriMesh::computeNormals (trimesh.cpp:608-676) as configure() applies it to a freshly loaded mesh."""
    if face_normals:
        normals = None
        if flip_normals:
            idx = idx[:, [1, 0, 2]]
    elif normals is not None:
        if flip_normals:
            normals = -normals
    else:
        normals = compute_normals(pos, idx, flip_normals)
    return normals, idx


def load_serialized(path, to_world=None, shape_index=0, face_normals=False, flip_normals=False, max_smooth_angle=None):
    """shapes/serialized.cpp:148-212 + TriMesh::loadCompressed (trimesh.cpp:175-295): Mitsuba's binary mesh format — header 0x041C,
    version 3 or 4, then a zlib stream {flags, [name], vertex count, triangle count, positions, [normals], [texcoords], [colours],
    indices}; several meshes per file are addressed through the offset table at the end (`shapeIndex`)."""
    import struct
    import zlib
    to_world = np.eye(4, dtype=f32) if to_world is None else to_world
    buf = open(path, "rb").read()

    def header(off):
        fmt, version = struct.unpack_from("<HH", buf, off)
        if fmt != 0x041C:
            raise SceneError("%s: encountered an invalid file format!" % path)
        if version not in (3, 4):
            raise SceneError("%s: encountered an incompatible file version!" % path)
        return version
    version = header(0)
    start = 0
    if shape_index != 0:  # readOffset, trimesh.cpp:272-295
        if len(buf) < 8:
            raise SceneError("%s: truncated file" % path)
        count = struct.unpack_from("<I", buf, len(buf) - 4)[0]
        if shape_index < 0 or shape_index >= count:  # (the reference accepts shapeIndex == count and then reads past the offset table)
            raise SceneError("%s: shape index is out of range! (requested %d out of 0..%d)" % (path, shape_index, count - 1))
        back = (8 if version == 4 else 4) * (count - shape_index) + 4
        if back > len(buf):
            raise SceneError("%s: corrupt offset table" % path)
        start = struct.unpack_from("<Q" if version == 4 else "<I", buf, len(buf) - back)[0]
        if start + 4 > len(buf):
            raise SceneError("%s: corrupt offset table" % path)
        header(start)
    try:
        data = zlib.decompressobj().decompress(buf[start + 4:])
    except zlib.error as e:
        raise SceneError("%s: %s" % (path, e))
    off = 0
    flags = struct.unpack_from("<I", data, off)[0]; off += 4
    if version == 4:
        off = data.index(b"\0", off) + 1
    if off + 16 > len(data):
        raise SceneError("%s: truncated mesh data" % path)
    nv, nt = struct.unpack_from("<QQ", data, off); off += 16
    if nv > len(data) or nt > len(data):
        raise SceneError("%s: truncated mesh data" % path)
    dt = "<f8" if flags & 0x2000 else "<f4"

    def take(n_comp):
        nonlocal off
        if off + nv * n_comp * (8 if flags & 0x2000 else 4) > len(data):
            raise SceneError("%s: truncated mesh data" % path)
        a = np.frombuffer(data, dt, nv * n_comp, off).reshape(nv, n_comp).astype(f32)
        off += a.shape[0] * n_comp * (8 if flags & 0x2000 else 4)
        return a
    pos = take(3)
    normals = take(3) if flags & 0x0001 else None
    uvs = take(2) if flags & 0x0002 else None
    if flags & 0x0008:
        take(3)  # vertex colours: not used
    if off + nt * 12 > len(data):
        raise SceneError("%s: truncated mesh data" % path)
    idx = np.frombuffer(data, "<u4", nt * 3, off).reshape(nt, 3).astype(np.uint32)
    if idx.size and idx.max() >= nv:
        raise SceneError("%s: vertex index out of bounds" % path)
    if not np.array_equal(to_world, np.eye(4, dtype=f32)):
        pos = _xf_points(to_world, pos)
        if normals is not None:
            normals = _xf_normals(to_world, normals)
            normals = (normals / np.sqrt(np.sum(normals * normals, 1, dtype=f32), dtype=f32)[:, None]).astype(f32)
    if np.linalg.det(to_world[:3, :3].astype(np.float64)) < 0:
        idx = idx[:, [1, 0, 2]]
    if max_smooth_angle is not None:
        pos, uvs, idx = rebuild_topology(pos, uvs, idx, max_smooth_angle)
        normals = None
    normals, idx = _finish_normals(pos, normals, idx, face_normals, flip_normals)
    return dict(name=os.path.splitext(os.path.basename(path))[0], material="", positions=pos, normals=normals, indices=idx)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_ply(path, to_world=None, face_normals=False, flip_normals=False, max_smooth_angle=None):
    """shapes/ply.cpp: Stanford PLY (ascii / binary little / big endian) with vertex x y z [nx ny nz] [u v | s t] and faces of 3 or 4 indices
    (a quad becomes (0, 1, 2), (3, 0, 2), ply.cpp:299-311); positions and normals go through toWorld as they are read (:229-233)."""
    to_world = np.eye(4, dtype=f32) if to_world is None else to_world
    buf = open(path, "rb").read()
    end = buf.find(b"end_header")
    if not buf.startswith(b"ply") or end < 0:
        raise SceneError("%s: not a PLY file" % path)
    head = buf[:end].decode("latin1").splitlines()
    data_off = buf.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in head[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            elements[-1][2].append((tok[-1], tok[1:-1]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise SceneError("%s: unknown PLY format %r" % (path, fmt))
    verts, faces = {}, []
    if fmt == "ascii":
        tokens = iter(buf[data_off:].split())
        nxt = lambda typ: (float if _PLY_TYPES[typ][0] == "f" else int)(next(tokens))  # noqa: E731
    else:
        bo = "<" if fmt == "binary_little_endian" else ">"
        pos = [data_off]

        def nxt(typ):
            dt = np.dtype(bo + _PLY_TYPES[typ])
            v = np.frombuffer(buf, dt, 1, pos[0])[0]
            pos[0] += dt.itemsize
            return v
    for name, count, props in elements:
        cols = {pn: [] for pn, _ in props} if name == "vertex" else None
        for _ in range(count):
            for pn, ptype in props:
                if ptype[0] == "list":
                    n = int(nxt(ptype[1]))
                    vals = [int(nxt(ptype[2])) for _ in range(n)]
                    if name == "face" and pn in ("vertex_indices", "vertex_index"):
                        if n not in (3, 4):
                            raise SceneError("%s: only triangle and quad-based PLY meshes are supported" % path)
                        faces.append((vals[0], vals[1], vals[2]))
                        if n == 4:
                            faces.append((vals[3], vals[0], vals[2]))
                else:
                    v = nxt(ptype[0])
                    if cols is not None:
                        cols[pn].append(v)
        if name == "vertex":
            verts = cols
    if not faces or not verts or "x" not in verts:
        raise SceneError("Unable to load \"%s\" (no triangles or vertices found)!" % path)
    P = np.stack([np.asarray(verts[k], f32) for k in "xyz"], 1)
    N = np.stack([np.asarray(verts[k], f32) for k in ("nx", "ny", "nz")], 1) if all(k in verts for k in ("nx", "ny", "nz")) else None
    uvs = None
    for a, b in (("u", "v"), ("s", "t")):
        if a in verts and b in verts:
            uvs = np.stack([np.asarray(verts[a], f32), np.asarray(verts[b], f32)], 1)
    idx = np.asarray(faces, np.uint32)
    if idx.max() >= len(P):
        raise SceneError("%s: vertex index out of bounds" % path)
    pos_w = _xf_points(to_world, P)
    nrm_w = None
    if N is not None:
        nrm_w = _xf_normals(to_world, N)
        nrm_w = (nrm_w / np.sqrt(np.sum(nrm_w * nrm_w, 1, dtype=f32), dtype=f32)[:, None]).astype(f32)
    if max_smooth_angle is not None:
        pos_w, uvs, idx = rebuild_topology(pos_w, uvs, idx, max_smooth_angle)
        nrm_w = None
    nrm_w, idx = _finish_normals(pos_w, nrm_w, idx, face_normals, flip_normals)
    return dict(name=os.path.splitext(os.path.basename(path))[0], material="", positions=pos_w, normals=nrm_w, indices=idx)


def cube_mesh(to_world, flip_normals=False):
    """shapes/cube.cpp:24-30, 73-103: the cube [-1, 1]^3 as 6 faces x 4 vertices (own normals per face) and 12 triangles.  Face order
    -y, +y, +x, +z, -x, -z; a face's corners start at the corner given below and turn counter-clockwise about the face normal;
    triangles (0, 1, 2), (3, 0, 2) per face — the layout of the reference's vertex table."""
    faces = [((0, -1, 0), (1, -1, -1)), ((0, 1, 0), (1, 1, -1)), ((1, 0, 0), (1, -1, -1)), ((0, 0, 1), (1, -1, 1)), ((-1, 0, 0), (-1, -1, 1)),
             ((0, 0, -1), (1, 1, -1))]
    P, N, I = [], [], []
    for f, (n, start) in enumerate(faces):
        n, p = np.array(n, np.float64), np.array(start, np.float64)
        for _ in range(4):
            P.append(p); N.append(n)
            p = np.cross(n, p) + np.dot(n, p) * n          # a quarter turn about the normal
        I += [(4 * f, 4 * f + 1, 4 * f + 2), (4 * f + 3, 4 * f, 4 * f + 2)]
    pos = _xf_points(to_world, np.asarray(P, f32))
    nrm = _xf_normals(to_world, np.asarray(N, f32))
    nrm = (nrm / np.sqrt(np.sum(nrm * nrm, 1, dtype=f32), dtype=f32)[:, None]).astype(f32)
    if flip_normals:  # TriMesh::computeNormals with existing normals (trimesh.cpp:612-618)
        nrm = -nrm
    return dict(name="cube", material="", positions=pos, normals=nrm, indices=np.asarray(I, np.uint32))


def _props(elem, sub):
    out = {}
    for c in elem:
        n = c.get("name")
        if c.tag == "boolean":
            out[n] = sub(c.get("value")).strip().lower() == "true"
        elif c.tag == "integer":
            out[n] = int(sub(c.get("value")))
        elif c.tag == "float":
            out[n] = float(sub(c.get("value")))
        elif c.tag == "string":
            out[n] = sub(c.get("value"))
        elif c.tag == "point":
            out[n] = tuple(float(sub(c.get(k, "0"))) for k in "xyz")
    return out


def parse_rfilter(elem, sub=lambda v: v):
    """<rfilter type=...> of an hdrfilm (mitsuba/src/rfilters/): a SceneDesc.rfilter dict, None for the default box (radius 0.5).
    Parameters and defaults are Mitsuba's; an unknown type or parameter, or a value the filter cannot take, raises."""
    t = elem.get("type")
    allowed = dict(box={"radius": "float"}, tent={}, gaussian={"stddev": "float"}, mitchell={"B": "float", "C": "float"}, catmullrom={},
                   lanczos={"lobes": "integer"})
    if t not in allowed:
        raise SceneError("rfilter type %r is not supported (box, tent, gaussian, mitchell, catmullrom, lanczos)" % (t,))
    out = {"type": t}
    for c in elem:
        if not isinstance(c.tag, str):
            continue  # comments
        n = c.get("name")
        if n not in allowed[t] or c.tag != allowed[t][n]:
            raise SceneError("rfilter %r: unsupported parameter <%s name=%r>" % (t, c.tag, n))
        try:
            out[n] = int(sub(c.get("value"))) if c.tag == "integer" else float(sub(c.get("value")))
        except (TypeError, ValueError):
            raise SceneError("rfilter %r: bad value %r for %r" % (t, c.get("value"), n))
    bad = ((t == "box" and not out.get("radius", 0.5) > 0) or (t == "gaussian" and not out.get("stddev", 0.5) > 0) or
           (t == "lanczos" and out.get("lobes", 3) < 1) or any(not math.isfinite(v) for k, v in out.items() if k != "type"))
    if bad:
        raise SceneError("rfilter %r: parameter out of range: %r" % (t, out))
    from .bindings import RFilter
    desc = RFilter.from_dict(out).as_dict()  # (None for the default box)
    if _rfilter_border(RFilter.from_dict(out)) > 3:
        raise SceneError("rfilter %r: radius too large (more than 7x7 pixels per sample): %r" % (t, out))
    return desc


def _rfilter_border(f):
    """m_borderSize = ceil(radius - 0.5) of ReconstructionFilter::configure (rfilter.cpp:37-55), radius as the filters set it"""
    f32 = np.float32
    t = f.TYPES[f.type]
    r = {"box": f32(f.radius) + f32(1e-5), "tent": f32(1), "gaussian": f32(4) * f32(f.stddev), "mitchell": f32(2), "catmullrom": f32(2),
         "lanczos": f32(f.lobes)}[t]
    return int(np.ceil(f32(r) - f32(0.5)))


def focal_length_fov(text):
    """focalLength "<x>mm" → the diagonal field of view it stands for (PerspectiveCamera::configure, sensor.cpp:264-276), in the
    reference's float arithmetic: 2 · 180/π · atan(√(36² + 24²) / (2x))"""
    f = text[:-2] if text.endswith("mm") else text
    try:
        value = f32(float(f))
    except ValueError:
        raise SceneError("could not parse the focal length %r (must be of the form <x>mm, where <x> is a positive number)" % text)
    a = f32(np.arctan(f32(np.sqrt(f32(36 * 36 + 24 * 24))) / (f32(2) * value)))
    return float(f32(2 * 180 / math.pi * float(a)))


def _has_scale(m):
    """Transform::hasScale (transform.h:76-90): the rows of the 3x3 part are not orthonormal within 1e-3"""
    m = np.asarray(m, f32).reshape(4, 4)
    for i in range(3):
        for j in range(i, 3):
            acc = f32(0)
            for k in range(3):
                acc = f32(acc + m[i, k] * m[j, k])
            if (i == j and abs(acc - f32(1)) > f32(1e-3)) or (i != j and abs(acc) > f32(1e-3)):
                return True
    return False


def inverse3(m):
    """Inverse of the upper 3x3 of `m` by cofactors in double, rounded to float (host/scene_xml.h inverse3: the same operations)"""
    a, b, c, d, e, f, g, h, i = (float(m[r][k]) for r in range(3) for k in range(3))
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return np.array([(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det, (f * g - d * i) / det, (a * i - c * g) / det,
                     (c * d - a * f) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det], np.float64).astype(f32)


def parse_delta_emitter(em, rd):
    """<emitter type="point" | "spot" | "directional"> (mitsuba/src/emitters/point.cpp:57-69, spot.cpp:68-94, directional.cpp:55-73) → a
    SceneDesc.delta_emitters dict (bindings.DeltaEmitter).  `rd` is the load's reader (a spectrum property defaults to 1: the loader's D65)."""
    t = em.get("type")
    ep = _props(em, rd.sub)
    for c in em:
        if c.tag == "vector":
            ep[c.get("name")] = tuple(float(rd.sub(c.get(k, "0"))) for k in "xyz")
    tw = next((c for c in em if c.tag == "transform" and c.get("name", "toWorld") == "toWorld"), None)
    m = _transform(tw, rd.sub) if tw is not None else np.eye(4, dtype=f32)
    if float(ep.get("samplingWeight", 1.0)) != 1.0:
        raise SceneError("%s emitter: a samplingWeight other than 1 is not supported" % t)
    if t == "point":
        if "position" in ep and tw is not None:
            raise SceneError("point emitter: only one of the parameters 'position' and 'toWorld' can be used")
        pos = ep["position"] if "position" in ep else (m[0, 3], m[1, 3], m[2, 3])
        return dict(type="point", intensity=tuple(float(v) for v in rd._colour(em, "intensity", 1.0)), position=tuple(float(f32(v)) for v in pos))
    if t == "spot":
        if any(c.get("name") == "texture" or c.tag == "texture" for c in em):
            raise SceneError("spot emitter: a projection 'texture' is not supported")
        rad = f32(f32(math.pi) / f32(180))  # degToRad, util.h
        cutoff_deg = f32(ep.get("cutoffAngle", 20.0))
        beam_deg = f32(ep["beamWidth"]) if "beamWidth" in ep else f32(f32(cutoff_deg * f32(3)) / f32(4))
        cutoff, beam = f32(cutoff_deg * rad), f32(beam_deg * rad)
        if cutoff < beam:
            raise SceneError("spot emitter: cutoffAngle must not be smaller than beamWidth")
        if not (0 < beam and cutoff_deg < 90):
            raise SceneError("spot emitter: the angles must satisfy 0 < beamWidth <= cutoffAngle < 90 degrees")
        return dict(type="spot", intensity=tuple(float(v) for v in rd._colour(em, "intensity", 1.0)), position=(float(m[0, 3]), float(m[1, 3]), float(m[2, 3])),
                    to_local=[float(v) for v in inverse3(m)], cutoff_angle=float(cutoff), beam_width=float(beam))
    if "direction" in ep and tw is not None:
        raise SceneError("directional emitter: only one of the parameters 'direction' and 'toWorld' can be used at a time")
    if "direction" in ep:
        x, y, z = (f32(v) for v in ep["direction"])
        ln = f32(np.sqrt(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))))
        if not ln > 0:
            raise SceneError("directional emitter: 'direction' is zero")
        d = (float(f32(x / ln)), float(f32(y / ln)), float(f32(z / ln)))
    else:
        if _has_scale(m):
            raise SceneError("directional emitter: scale factors in the emitter-to-world transformation are not allowed")
        d = (float(m[0, 2]), float(m[1, 2]), float(m[2, 2]))
    return dict(type="directional", intensity=tuple(float(v) for v in rd._colour(em, "irradiance", 1.0)), direction=d)


def _decode_bitmap(full, channel, gamma):
    """The float32 `rgb` texels of an image file and, where they are its own sRGB encoding decoded, the 8-bit texels as `srgb8`: 8-bit files go
    through the sRGB curve unless `gamma` says otherwise (bitmap.cpp:182-204), luminance and a single `channel` are replicated to RGB"""
    from . import imageio
    from .scenes import srgb8_table
    if os.path.splitext(full)[1].lower() in (".exr", ".pfm", ".hdr", ".rgbe"):
        rgb = np.ascontiguousarray(imageio.read_image(full), f32)  # floating point data is linear (bitmap.cpp:190-192)
        if channel:  # a monochrome texture of that channel (bitmap.cpp:238-256)
            if channel == "a":
                raise SceneError("bitmap: '%s' has no channel 'a' (channels present: r, g, b)" % full)
            rgb = np.ascontiguousarray(np.repeat(rgb[:, :, "rgb".index(channel)][:, :, None], 3, 2))
        return dict(rgb=rgb)
    try:
        from PIL import Image
    except ImportError:
        raise SceneError("bitmap: decoding '%s' needs PIL (scene conversion only)" % full)
    im = Image.open(full)
    if channel:  # one channel of the file as a monochrome texture, replicated to RGB (bitmap.cpp:238-256)
        if im.mode in ("P", "CMYK", "1"):
            im = im.convert("RGBA" if "transparency" in im.info else "RGB")
        names = {"L": "y", "LA": "ya", "RGB": "rgb", "RGBA": "rgba"}.get(im.mode)
        a = np.asarray(im)
        if names is None or a.dtype != np.uint8:
            raise SceneError("bitmap: '%s': only 8-bit images are decoded here" % full)
        if channel not in names:
            raise SceneError("bitmap: '%s' has no channel %r (channels present: %s)" % (full, channel, ", ".join(names)))
        a = np.ascontiguousarray(np.repeat(a.reshape(a.shape[0], a.shape[1], -1)[:, :, names.index(channel)][:, :, None], 3, 2))
        gamma = 1.0 if channel == "a" else gamma  # alpha is never gamma-corrected (bitmap.cpp:258-263)
        if gamma == 1.0:
            return dict(rgb=(a.astype(f32) / f32(255.0)).astype(f32))
    else:
        if im.mode in ("P", "RGBA", "LA", "CMYK", "1", "I;16", "I"):  # alpha is dropped for a spectrum texture (bitmap.cpp:218-236: EAuto → RGB / luminance)
            im = im.convert("RGB" if im.mode != "LA" else "L")
        a = np.asarray(im)
        if a.dtype != np.uint8:
            raise SceneError("bitmap: '%s': only 8-bit images are decoded here" % full)
        if a.ndim == 2:
            a = np.repeat(a[:, :, None], 3, 2)
        a = np.ascontiguousarray(a[:, :, :3])
    if gamma == 0.0 or gamma == -1.0:  # the file's own encoding: sRGB for 8-bit images
        return dict(srgb8=a, rgb=srgb8_table()[a])
    # an explicit gamma (bump maps ask for 1.0, bumpmap.cpp:121-126): value^gamma on value / 255
    return dict(rgb=np.power(a.astype(np.float64) / 255.0, gamma).astype(f32))


# ---------------------------------------------------------------------------------------------- what several readers ask of an element or a material
_nested_bsdfs = lambda elem: [c for c in elem if c.tag == "bsdf"]  # noqa: E731
_texture_on = lambda elem, *names: any(c.get("name") in names and c.tag in ("texture", "ref") for c in elem)  # noqa: E731 (a <texture> or <ref> on one of them)
_stated = lambda elem, name: any(c.get("name") == name for c in elem)  # noqa: E731
_blend_children = lambda m: [c for c in (m.get("blend") or {}).get("children", ()) if isinstance(c, dict)]  # noqa: E731
_IOR = {"vacuum": 1.0, "air": 1.000277, "water": 1.3330, "polypropylene": 1.49, "bk7": 1.5046, "diamond": 2.419}  # well-known constants (cf. ior.h)


def _lookup_ior(p, name, default):  # lookupIOR, ior.h:95-111: a number or a material name
    v = p.get(name, default)
    if isinstance(v, (int, float)):
        return float(v)
    if str(v).lower() not in _IOR:
        raise SceneError("IOR name %r is not in the built-in list %s; give a number" % (v, sorted(_IOR)))
    return _IOR[str(v).lower()]


def _dielectric_eta(p, what, int_default):  # intIOR / extIOR of the rough plug-ins (roughdielectric.cpp:183-211, roughplastic.cpp:197-227)
    int_ior, ext_ior = _lookup_ior(p, "intIOR", int_default), _lookup_ior(p, "extIOR", "air")
    if int_ior < 0 or ext_ior < 0 or int_ior == ext_ior:
        raise SceneError("%s: the interior and exterior indices of refraction must be positive and differ" % what)
    return float(f32(int_ior / ext_ior))


def _freeze(v):  # a material dict's value as something hashable
    if isinstance(v, dict):
        return tuple(sorted((a, _freeze(b)) for a, b in v.items()))
    return tuple(_freeze(x) for x in v) if isinstance(v, (tuple, list)) else v


def _reads_bitmap(m):  # whether the material, the weight of its blend or a child of it reads a bitmap at the hit's uv
    return (any(k in m for k in TEXTURE_KEYS) or (m.get("blend") or {}).get("weight_texture") is not None
            or any(_reads_bitmap(c) for c in _blend_children(m)))


def _anisotropic(m):
    """EAnisotropic: alphaU != alphaV, or either a bitmap — in the material or in a child of its blend.  Needs the UV tangents (trimesh.cpp:380, 683-735)."""
    own = m.get("alpha_v") is not None and (max(f32(m["alpha_v"]), f32(1e-4)) != max(f32(m.get("alpha", 0.1)), f32(1e-4))
                                            or m.get("alpha_texture") is not None or m.get("alpha_v_texture") is not None)
    return own or any(_anisotropic(c) for c in _blend_children(m))


# ---------------------------------------------------------------------------------------------- the state of one load
class _Reader:
    """One load_scene() call: the state its readers share, and the readers as methods.  The tables only grow, in the order in which the
    scene file names their entries: materials and textures are referred to by index."""

    def __init__(self, root, path, defines, strict, data_dir, mitsuba_src):
        self.params = dict(defines or {})  # -D name=value, then the file's <default>s
        for d in root.iter("default"):
            self.params.setdefault(d.get("name"), d.get("value"))
        self.strict, self.warnings = strict, []  # refuse what cannot be rendered, or substitute or skip it and say so in `warnings`
        self.base = os.path.dirname(os.path.abspath(path))  # relative file names start here
        self.data_dir, self.mitsuba_src = data_dir, mitsuba_src
        self.tex_by_id = {t.get("id"): t for t in root.findall("texture") if t.get("id")}  # top-level <texture id> elements, for <ref>
        self.textures, self.tex_index, self.scaled_index = [], {}, {}  # SceneDesc.textures; bitmap key → index; (index, factor) → index of the scaled copy
        self.materials, self.mat_index, self.by_id = [], {}, {}  # material dicts; frozen dict → index; bsdf id → index
        self.rt_slices, self.rt_index = [], {}  # rough-transmittance slices; (distribution, alpha, eta) → index
        self.media, self.medium_by_id = [], {}  # medium dicts (bindings.Medium); medium id → index, or None for one a lenient load dropped

    def sub(self, text):  # $name → its -D or <default> value (mitsuba.cpp:58-87)
        if text is None or "$" not in text:
            return text
        for k in re.findall(r"\$(\w+)", text):
            if k not in self.params:
                raise SceneError("undefined parameter $%s (pass it with -D %s=...)" % (k, k))
        return re.sub(r"\$(\w+)", lambda mo: str(self.params[mo.group(1)]), text)

    def _colour(self, elem, name, default):  # the rgb of the spectrum property `name` of `elem`, `default` in all three channels where it is absent
        for c in elem:
            if c.get("name") == name:
                if c.tag in ("rgb", "srgb", "spectrum"):
                    if c.get("filename"):  # InterpolatedSpectrum(path) (spectrum.cpp:575-600): "wavelength value" lines, # comments
                        fn = self.sub(c.get("filename"))
                        full = fn if os.path.isabs(fn) else os.path.join(self.base, fn)
                        if c.tag != "spectrum" or c.get("value") is not None or not os.path.exists(full):
                            raise SceneError("<%s filename=%r>: %s" % (c.tag, fn, "file not found" if c.tag == "spectrum" and c.get("value") is None
                                                                         else "please provide one of 'value' or 'filename'"))
                        pairs = spectrum.read_spd(full)
                        if len(pairs) < 2:
                            raise SceneError("<spectrum filename=%r>: fewer than two samples" % fn)
                        return spectrum.interpolated_to_rgb(pairs)
                    return spectrum.parse(c.tag, self.sub(c.get("value")))
                if c.tag == "blackbody":
                    t = self.sub(c.get("temperature", "")).strip()
                    return spectrum.blackbody_to_rgb(float(t[:-1] if t[-1:] in "kK" else t), float(self.sub(c.get("scale", "1"))))
                if c.tag == "texture" or c.tag == "ref":
                    if self.strict:
                        raise SceneError("a texture on %r is not supported (bitmaps on reflectances, specular colours, roughconductor / roughdielectric alpha, mask opacity and bump maps are)" % name)
                    self.warnings.append("texture on %r ignored: the plug-in's default value is used" % name)
                    break
        return np.full(3, default, f32)

    def _bitmap_texture(self, elem, what):
        """<texture type="bitmap"> (textures/bitmap.cpp:90-330) → index into `self.textures`.  The image is decoded here because the integrator only
        ever reads level 0 of the MIP map (include/ppg.h ppg_texture)."""
        if elem.tag == "ref":
            target = self.tex_by_id.get(elem.get("id"))
            if target is None:
                raise SceneError("<ref id=%r>: no such texture" % elem.get("id"))
            elem = target
        if elem.get("type") == "scale":
            return self._scaled_texture(elem, what)
        if elem.get("type") != "bitmap":
            raise SceneError("texture type %r on %s is not supported (bitmap only)" % (elem.get("type"), what))
        tp = _props(elem, self.sub)
        fn = tp.get("filename")
        if not fn:
            raise SceneError("bitmap texture without filename")
        full = fn if os.path.isabs(fn) else os.path.join(self.base, fn)
        wrap = str(tp.get("wrapMode", "repeat")).lower()
        wu, wv = str(tp.get("wrapModeU", wrap)).lower(), str(tp.get("wrapModeV", wrap)).lower()
        for wm in (wu, wv):
            if wm not in ("repeat", "mirror", "clamp", "zero", "one"):
                raise SceneError("bitmap: invalid wrap mode %r" % wm)  # bitmap.cpp:113-127
        filt = str(tp.get("filterType", "ewa")).lower()
        if filt not in ("ewa", "trilinear", "nearest", "bilinear"):
            raise SceneError("bitmap: invalid filter type %r" % filt)
        gamma = float(tp.get("gamma", 0.0))
        su, sv, ou, ov = (float(tp.get(k, d)) for k, d in (("uscale", 1.0), ("vscale", 1.0), ("uoffset", 0.0), ("voffset", 0.0)))
        key = (full, wu, wv, filt == "nearest", gamma, su, sv, ou, ov, str(tp.get("channel", "")))
        if key in self.tex_index:
            return self.tex_index[key]
        if not os.path.exists(full):
            raise SceneError("bitmap: file '%s' not found" % full)
        channel = str(tp.get("channel", "")).lower()
        if channel and channel not in ("r", "g", "b", "a"):
            raise SceneError("bitmap: channel %r is not supported (r, g, b, a)" % tp.get("channel"))
        t = dict(uv_scale=(su, sv), uv_offset=(ou, ov), wrap_u=wu, wrap_v=wv, nearest=filt == "nearest", source=os.path.basename(full))
        t.update(_decode_bitmap(full, channel, gamma))
        # Texture::getAverage: the mean of the full-resolution image (the MIP map's 1x1 level; exact for power-of-two sizes)
        t["average"] = [float(v) for v in t["rgb"].reshape(-1, 3).mean(0, dtype=np.float64)]
        self.tex_index[key] = len(self.textures)
        self.textures.append(t)
        return self.tex_index[key]

    def _scaled_texture(self, elem, what):
        """<texture type="scale"> (textures/scale.cpp:50-156) around one bitmap, or around a scale around one → index into `self.textures` of a
        texture of its own whose texels are the nested one's times the factor, in float32: what ScalingTexture::getBitmap does.  Its
        average and a bump map's gradient scale with it.  (Mitsuba scales the interpolated value; the two differ by rounding only.)"""
        tp = _props(elem, self.sub)
        if any(c.get("name") == "scale" and c.tag in ("rgb", "srgb", "spectrum", "blackbody") for c in elem):
            factor = np.asarray(self._colour(elem, "scale", 1.0), f32)
        else:
            try:
                factor = np.full(3, f32(float(tp.get("scale", 1.0))), f32)
            except (TypeError, ValueError):
                raise SceneError("scale: could not parse the scale factor %r" % (tp.get("scale"),))
        if not (np.isfinite(factor).all() and (factor > 0).all()):  # Assert(m_scale.min() > 0), scale.cpp:62
            raise SceneError("scale: the scale factor must be finite and > 0 (got %s)" % ", ".join(repr(float(v)) for v in factor))
        nested = [c for c in elem if c.tag == "texture" or (c.tag == "ref" and c.get("id") in self.tex_by_id)]
        if "value" in tp or any(c.get("name") == "value" for c in elem):
            raise SceneError("scale: a constant 'value' inside a scale texture is not supported (a bitmap, or a scale around one, is)")
        if not nested:
            raise SceneError("scale: The scale plugin needs a nested texture!")  # scale.cpp:73-74
        if len(nested) > 1:
            raise SceneError("scale: exactly one nested texture is required (found %d)" % len(nested))
        inner = self.tex_by_id[nested[0].get("id")] if nested[0].tag == "ref" else nested[0]
        if inner.get("type") not in ("bitmap", "scale"):
            raise SceneError("scale: texture type %r inside a scale texture is not supported (a bitmap, or a scale around one, is)" % inner.get("type"))
        ti = self._bitmap_texture(inner, what)
        src = self.textures[ti]
        if "one" in (src["wrap_u"], src["wrap_v"]):
            raise SceneError("scale around a bitmap with wrap mode 'one' is not supported: the constant outside the image would not scale")
        key = (ti,) + tuple(float(v) for v in factor)
        if key not in self.scaled_index:
            rgb = np.ascontiguousarray(src["rgb"] * factor, f32)
            self.textures.append(dict({k: v for k, v in src.items() if k != "srgb8"}, rgb=rgb,
                                    average=[float(v) for v in rgb.reshape(-1, 3).mean(0, dtype=np.float64)]))
            self.scaled_index[key] = len(self.textures) - 1
        return self.scaled_index[key]

    def _is_texture(self, c):  # whether the child element is a <texture>, or a <ref> to a top-level one
        return c.tag == "texture" or (c.tag == "ref" and c.get("id") in self.tex_by_id)

    def _colour_or_texture(self, elem, name, default, wrap=False):
        """(rgb, texture index or None) of a parameter that may be a bitmap; rgb is then the bitmap's average.  `wrap`: a loader failure is
        reported as "texture on <name>: ..." (the parameters other than the diffuse reflectance)."""
        for c in elem:
            if c.get("name") == name and self._is_texture(c):
                try:
                    ti = self._bitmap_texture(c, name)
                except SceneError as e:
                    if self.strict:
                        if wrap:
                            raise SceneError("texture on %r: %s" % (name, e))
                        raise
                    self.warnings.append("texture on %r ignored (%s): the plug-in's default value is used" % (name, e))
                    return np.full(3, default, f32), None
                return np.asarray(self.textures[ti]["average"], f32), ti
        return self._colour(elem, name, default), None

    def _textured(self, elem, m, name, d, field="reflectance", key="texture"):  # m[field] = the colour `name`; a bitmap on it gives its average, and its index as m[key]
        c, ti = self._colour_or_texture(elem, name, d, wrap=name != "reflectance" and name != "diffuseReflectance")
        m[field] = tuple(float(v) for v in c)
        if ti is not None:
            m[key] = ti
        return m

    def _specular(self, elem, m, name):  # the `specular` field: plastic specularReflectance, dielectric specularTransmittance
        return self._textured(elem, m, name, 1.0, "specular", "specular_texture")

    def _alpha_value(self, elem, p, tex, name):  # (a roughness, its texture index or None): a number, or a bitmap read as eval(its).average(), the constant
        if name not in tex:
            return float(p[name]), None
        c, ti = self._colour_or_texture(elem, name, 0.1, wrap=True)
        return float((f32(c[0]) + f32(c[1]) + f32(c[2])) / f32(3.0)), ti  # Spectrum::average (spectrum.h:481-486)

    def _microfacet(self, elem, p, m, what):
        """MicrofacetDistribution(props) (microfacet.h:99-145) plus the plug-ins' texture children on alpha / alphaU / alphaV: fills the
        material's alpha (alphaU) and, where the BSDF states alphaU / alphaV, phong or sampleVisible = false, the keys of the general entry
        (alpha_v, alpha_v_texture, distribution = "phong", sample_visible = False; bindings.Microfacet)."""
        distr = str(p.get("distribution", "beckmann")).lower()
        if distr not in ("beckmann", "ggx", "phong", "as"):
            raise SceneError('%s: Specified an invalid distribution "%s", must be "beckmann", "ggx", or "phong"/"as"!' % (what, distr))
        if distr in ("phong", "as") and what not in ("roughplastic", "roughcoating"):
            # the XML loaders read the Phong / Ashikhmin-Shirley distribution on roughplastic only: tests/test_mitsuba_xml.py pins its refusal
            # on roughconductor.  The other two plug-ins get it through material dicts, flat scene files and the C-ABI.
            raise SceneError("%s: distribution %r is not supported by the scene loaders on this plug-in (ggx, beckmann; phong on roughplastic)" % (what, distr))
        tex = {c.get("name") for c in elem if c.tag in ("texture", "ref")} & {"alpha", "alphaU", "alphaV"}
        has = lambda n: n in p or n in tex  # noqa: E731
        if has("alpha"):
            if has("alphaU") or has("alphaV"):
                raise SceneError("%s: Microfacet model: please specify either 'alpha' or 'alphaU'/'alphaV'." % what)
            m["alpha"], ti = self._alpha_value(elem, p, tex, "alpha")
            if ti is not None:
                m["alpha_texture"] = ti
        elif has("alphaU") or has("alphaV"):
            if not has("alphaU") or not has("alphaV"):
                raise SceneError("%s: Microfacet model: both 'alphaU' and 'alphaV' must be specified." % what)
            m["alpha"], tu = self._alpha_value(elem, p, tex, "alphaU")
            m["alpha_v"], tv = self._alpha_value(elem, p, tex, "alphaV")
            if tu is not None:
                m["alpha_texture"] = tu
            if tv is not None:
                m["alpha_v_texture"] = tv
        else:
            m["alpha"] = 0.1
        if distr != "ggx":  # (beckmann is Mitsuba's default, microfacet.h:99)
            m["distribution"] = "beckmann" if distr == "beckmann" else "phong"
        if not p.get("sampleVisible", True):
            m["sample_visible"] = False
        return m

    def _conductor_ior(self, elem, p, what):  # conductor.cpp:160-186 / roughconductor.cpp:174-186
        ext = _lookup_ior(p, "extEta", "air")
        name = str(p.get("material", "Cu"))
        if name.lower() == "none":
            int_eta, int_k = np.zeros(3, f32), np.ones(3, f32)
        else:
            have = {c.get("name") for c in elem}
            int_eta = int_k = None
            if not ({"eta", "k"} <= have):  # the measured spectra ship with Mitsuba (data/ior/<name>.{eta,k}.spd), not with this repository
                ddir = self.data_dir or os.environ.get("PPG_MITSUBA_DATA")
                files = [os.path.join(ddir, "ior", "%s.%s.spd" % (name, part)) for part in ("eta", "k")] if ddir else []
                if not ddir or not all(os.path.exists(f) for f in files):
                    raise SceneError("%s(material=%s): the measured IOR spectra data/ior/%s.{eta,k}.spd come with Mitsuba: pass data_dir (--data-dir) / "
                                     "PPG_MITSUBA_DATA, or give <spectrum|rgb name=\"eta\"> and \"k\"" % (what, name, name))
                int_eta, int_k = (spectrum.interpolated_to_rgb(spectrum.read_spd(f), zero_extend=False, clamp=False) for f in files)
        eta = self._colour(elem, "eta", 0.0) if _stated(elem, "eta") else int_eta
        k = self._colour(elem, "k", 1.0) if _stated(elem, "k") else int_k
        return tuple(float(v) for v in (eta / f32(ext))), tuple(float(v) for v in (k / f32(ext)))  # roughconductor.cpp:185-186

    def _rt_slice(self, what, distr, alpha, eta):  # index into `self.rt_slices` of the rough-transmittance slice, read from Mitsuba's data/microfacet/<distr>.dat
        from . import rtrans
        key = (distr, float(f32(alpha)), eta)
        if key not in self.rt_index:
            try:
                self.rt_slices.append(rtrans.roughplastic_slice(distr, alpha, eta, self.data_dir))
            except rtrans.RoughTransmittanceError as e:
                raise SceneError("%s: %s" % (what, e))
            self.rt_index[key] = len(self.rt_slices) - 1
        return self.rt_index[key]

    def _conserve_energy(self, m, p, t, params):
        """BSDF::ensureEnergyConservation (bsdf.cpp:88-146) as the lobes' configure() calls it.  params: (Mitsuba's name, the dict's field, the key
        of its bitmap or None) — one, or the pair whose maxima are added.  A component-wise maximum above 1 scales them by 0.99 / max; a bitmap's
        maximum is taken over its texels, and a scaled bitmap is a texture of its own (the `scale` texture around it)."""
        if not p.get("ensureEnergyConservation", True):
            return m
        total = np.zeros(3, f32)
        for _, field, key in params:
            ti = m.get(key) if key else None
            total = total + (np.asarray(m[field], f32) if ti is None else self.textures[ti]["rgb"].reshape(-1, 3).max(0).astype(f32))
        actual = f32(total.max())
        if not actual > 1:
            return m
        scale = f32(0.99) * (f32(1.0) / actual)
        names = " and ".join('"%s"' % n for n, _, _ in params)
        self.warnings.append("bsdf %r violates energy conservation: %s %s a component-wise maximum of %s (> 1) and will be scaled by %s "
                             "(ensureEnergyConservation=false prevents this)" % (t, names, "has" if len(params) == 1 else "sum to", float(actual), float(scale)))
        for _, field, key in params:
            m[field] = tuple(float(f32(v) * scale) for v in m[field])
            if key and m.get(key) is not None:
                src = self.textures[m[key]]
                self.textures.append(dict({k: v for k, v in src.items() if k != "srgb8"}, rgb=np.ascontiguousarray(src["rgb"] * scale, f32),
                                          average=[float(f32(v) * scale) for v in src["average"]]))
                m[key] = len(self.textures) - 1
        return m

    def _unsupported_bsdf(self, t):  # where every reader that cannot make anything of its element ends: refused by name, or the lenient load's diffuse(0.5)
        if self.strict:
            raise SceneError("bsdf type %r is not supported yet (diffuse, roughdiffuse, difftrans, phong, conductor, roughconductor, plastic, roughplastic, dielectric, "
                             "thindielectric, roughdielectric, null, mask(...), twosided(...), bumpmap(...), normalmap(...); SURVEY.md §8 f1)" % t)
        self.warnings.append("bsdf %r replaced by diffuse(0.5)" % t)
        return dict(type=0, reflectance=(0.5, 0.5, 0.5), _substituted=True)

    def _read_twosided(self, elem, p, allow_twosided):
        inner = _nested_bsdfs(elem)
        if len(inner) != 1:
            return self._unsupported_bsdf("twosided(%s)" % ",".join(c.get("type", "?") for c in inner))
        m = self._make_bsdf(inner[0], allow_twosided=False)
        transmissive = {6: "dielectric", 7: "dielectric", 8: "dielectric", 11: "difftrans", 13: "null"}.get(m["type"])
        if transmissive:
            raise SceneError("twosided(%s): only BRDFs can be two-sided (twosided.cpp:84-88)" % transmissive)
        if m["type"] == 0 and not m.get("_substituted") and "blend" not in m:
            return dict({k: v for k, v in m.items() if k in TEXTURE_KEYS + ("coating",)}, type=1, reflectance=m["reflectance"])
        return dict(m, twosided=True)  # (a blended material's own record stays diffuse + two-sided: it only carries the adapters)

    def _read_mask(self, elem, p, allow_twosided):
        inner = _nested_bsdfs(elem)
        if len(inner) != 1:
            return self._unsupported_bsdf("mask(%s)" % ",".join(c.get("type", "?") for c in inner))
        m = self._make_bsdf(inner[0])
        if "opacity" in m:
            raise SceneError("mask(mask(...)) is not supported")
        if m["type"] == 13:
            raise SceneError("mask(null) is not supported")
        if m["type"] == 1:
            m = dict({k: v for k, v in m.items() if k in TEXTURE_KEYS + ("coating",)}, type=0, reflectance=m["reflectance"], twosided=True)
        return self._textured(elem, dict(m), "opacity", 0.5, "opacity", "opacity_texture")

    def _read_conductor(self, elem, p, allow_twosided):  # conductor and roughconductor
        t = elem.get("type")
        if t == "conductor" and str(p.get("material", "Cu")).lower() == "none":
            return self._textured(elem, dict(type=2), "specularReflectance", 1.0)
        eta, k = self._conductor_ior(elem, p, t)
        m = self._textured(elem, dict(type=3 if t == "conductor" else 4, eta=eta, k=k), "specularReflectance", 1.0)
        return m if t == "conductor" else self._microfacet(elem, p, m, t)

    def _read_plastic(self, elem, p, allow_twosided):
        eta = _lookup_ior(p, "intIOR", "polypropylene") / _lookup_ior(p, "extIOR", "air")
        m = self._specular(elem, dict(type=5, eta=float(f32(eta)), nonlinear=bool(p.get("nonlinear", False))), "specularReflectance")
        return self._textured(elem, m, "diffuseReflectance", 0.5)

    def _read_dielectric(self, elem, p, allow_twosided):  # dielectric and thindielectric
        eta = _lookup_ior(p, "intIOR", "bk7") / _lookup_ior(p, "extIOR", "air")
        m = self._textured(elem, dict(type=6 if elem.get("type") == "dielectric" else 7, eta=float(f32(eta))), "specularReflectance", 1.0)
        return self._specular(elem, m, "specularTransmittance")

    def _read_roughplastic(self, elem, p, allow_twosided):  # roughplastic.cpp:197-227, 285-305
        if _texture_on(elem, "alpha", "alphaU", "alphaV"):
            # its rough-transmittance slice is reduced to ONE alpha at conversion; a varying alpha needs the 2-D table (roughplastic.cpp:295-298)
            raise SceneError("roughplastic: a texture on 'alpha' is not supported (roughness maps are, on roughconductor and roughdielectric)")
        eta = _dielectric_eta(p, "roughplastic", "polypropylene")
        mf = self._microfacet(elem, p, {}, "roughplastic")
        if mf.get("alpha_v", mf["alpha"]) != mf["alpha"]:  # roughplastic.cpp:221-223
            raise SceneError("roughplastic: The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!")
        # (the distribution is also the name of its table, data/microfacet/<name>.dat)
        m = dict(mf, type=9, eta=eta, nonlinear=bool(p.get("nonlinear", False)), rtrans=self._rt_slice("roughplastic", mf.get("distribution", "ggx"), mf["alpha"], eta))
        return self._textured(elem, self._specular(elem, m, "specularReflectance"), "diffuseReflectance", 0.5)

    def _read_roughdielectric(self, elem, p, allow_twosided):
        m = self._textured(elem, dict(type=8, eta=_dielectric_eta(p, "roughdielectric", "bk7")), "specularReflectance", 1.0)
        return self._microfacet(elem, p, self._specular(elem, m, "specularTransmittance"), "roughdielectric")

    def _lobe_number(self, elem, p, name, default):  # a float32 parameter of roughdiffuse / phong that must be a constant
        if _texture_on(elem, name):
            if self.strict:
                raise SceneError("%s: a texture on %r is not supported (a bitmap on its reflectance is)" % (elem.get("type"), name))
            self.warnings.append("texture on %r ignored: the plug-in's default value is used" % name)
            return float(f32(default))
        return float(f32(p.get(name, default)))

    def _read_roughdiffuse(self, elem, p, allow_twosided):  # roughdiffuse.cpp:88-122
        old_name = _stated(elem, "diffuseReflectance") and not _stated(elem, "reflectance")
        m = self._textured(elem, dict(type=10, alpha=self._lobe_number(elem, p, "alpha", 0.2)), "diffuseReflectance" if old_name else "reflectance", 0.5)
        if p.get("useFastApprox", False):
            m["fast_approx"] = True
        return self._conserve_energy(m, p, "roughdiffuse", [("reflectance", "reflectance", "texture")])

    def _read_difftrans(self, elem, p, allow_twosided):  # difftrans.cpp:49-74
        old_name = _stated(elem, "diffuseTransmittance") and not _stated(elem, "transmittance")
        m = self._textured(elem, dict(type=11), "diffuseTransmittance" if old_name else "transmittance", 0.5)
        return self._conserve_energy(m, p, "difftrans", [("transmittance", "reflectance", "texture")])

    def _read_phong(self, elem, p, allow_twosided):  # phong.cpp:60-107: the colours may be bitmaps, the exponent and specularReflectance are constants
        if self.strict and _texture_on(elem, "specularReflectance"):
            raise SceneError("phong: a texture on 'specularReflectance' is not supported (a bitmap on its diffuseReflectance is)")
        m = dict(type=12, exponent=self._lobe_number(elem, p, "exponent", 30.0), specular=tuple(float(v) for v in self._colour(elem, "specularReflectance", 0.2)))
        m = self._textured(elem, m, "diffuseReflectance", 0.5)
        return self._conserve_energy(m, p, "phong", [("specularReflectance", "specular", None), ("diffuseReflectance", "reflectance", "texture")])

    def _read_coating(self, elem, p, allow_twosided):  # SmoothCoating (coating.cpp:109-200), RoughCoating (roughcoating.cpp:114-227): the innermost adapter
        t, inner = elem.get("type"), _nested_bsdfs(elem)
        try:
            return self._coated(elem, p, t, inner)
        except SceneError as e:
            if self.strict:
                raise
            if len(inner) != 1:
                return self._unsupported_bsdf(t)
            self.warnings.append("bsdf %r dropped around its nested bsdf (%s)" % (t, e))  # where a strict load refuses this coat, a lenient one renders the nested BSDF
            return self._make_bsdf(inner[0], allow_twosided)

    def _coated(self, elem, p, t, inner):  # the nested BSDF's dict with the adapter's parameters under `coating` (bindings.Coating); the plug-ins' parameters are constants
        if len(inner) != 1:
            raise SceneError("%s: exactly one nested bsdf is required (found %d)" % (t, len(inner)))
        it = inner[0].get("type")
        if it in ("coating", "roughcoating", "twosided", "mask", "bumpmap", "normalmap"):
            raise SceneError("%s(%s) is not supported: the nesting order is bumpmap(mask(twosided(coating(..))))" % (t, it))
        if it == "null":
            raise SceneError("%s(null): a coat on the null BSDF is not supported" % t)
        if it in ("blendbsdf", "mixturebsdf"):
            raise SceneError("%s(%s) is not supported: neither a coat around a blend nor a coated child" % (t, it))
        for c in elem:
            if c.tag in ("texture", "ref") and c.get("name") in ("sigmaA", "specularReflectance", "alpha", "alphaU", "alphaV"):
                raise SceneError("%s: a texture on %r is not supported" % (t, c.get("name")))
        m = self._make_bsdf(inner[0], allow_twosided=False)
        if m["type"] in (6, 7, 8):
            raise SceneError("%s(%s): a coat on dielectric, thindielectric or roughdielectric is not supported" % (t, it))
        if m["type"] in (10, 11, 12):
            raise SceneError("%s(%s): a coat on roughdiffuse, difftrans or phong is not supported" % (t, it))
        if t == "roughcoating" and m["type"] in (2, 3, 5):
            raise SceneError("roughcoating(%s): a roughcoating over a BSDF with a delta component (conductor, plastic) is not supported" % it)
        int_ior, ext_ior = _lookup_ior(p, "intIOR", "bk7"), _lookup_ior(p, "extIOR", "air")
        if int_ior < 0 or ext_ior < 0 or int_ior == ext_ior:
            raise SceneError("%s: The interior and exterior indices of refraction must be positive and differ!" % t)
        eta = float(f32(int_ior / ext_ior))
        thickness = float(f32(p.get("thickness", 1.0)))
        sigma_a = tuple(float(v) for v in self._colour(elem, "sigmaA", 0.0))
        spec = tuple(float(v) for v in self._colour(elem, "specularReflectance", 1.0))
        if not (eta > 0 and eta != 1.0):
            raise SceneError("%s: The interior and exterior indices of refraction must be positive and differ!" % t)
        if not all(math.isfinite(v) for v in (eta, thickness) + sigma_a + spec):
            raise SceneError("%s: a parameter is not finite" % t)
        if thickness < 0 or min(sigma_a) < 0:
            raise SceneError("%s: thickness and sigmaA must not be negative" % t)
        c = dict(kind=t, eta=eta, thickness=thickness, sigma_a=sigma_a, specular=spec)
        if t == "roughcoating":
            mf = self._microfacet(elem, p, {}, t)
            if mf.get("alpha_v", mf["alpha"]) != mf["alpha"]:  # roughcoating.cpp:143-145 (the plug-in's own words)
                raise SceneError("roughcoating: The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!")
            if not math.isfinite(mf["alpha"]):
                raise SceneError("roughcoating: a parameter is not finite")
            distr = mf.get("distribution", "ggx")
            c.update(alpha=float(f32(mf["alpha"])), distribution=distr, sample_visible=bool(mf.get("sample_visible", True)),
                     slice=self._rt_slice(t, distr, mf["alpha"], eta))  # the reduction roughplastic uses, interned with its slices
        return dict(m, coating=c)

    def _read_blend(self, elem, p, allow_twosided):  # BlendBSDF (blendbsdf.cpp:70-133), MixtureBSDF (mixturebsdf.cpp:64-172): where a leaf stands
        t = elem.get("type")
        try:
            return self._blended(elem, p, t)
        except SceneError as e:
            if self.strict:
                raise
            self.warnings.append("bsdf %r replaced by diffuse(0.5) (%s)" % (t, e))
            return dict(type=0, reflectance=(0.5, 0.5, 0.5), _substituted=True)

    def _blend_child(self, t, c):  # one child of a blend as a material dict: a nested <bsdf>, or a <ref> to a <bsdf> with an id that stands before it
        if c.tag == "ref":
            if c.get("id") not in self.by_id:
                raise SceneError('%s: <ref id="%s">: no such bsdf before it' % (t, c.get("id")))
            m, it = dict(self.materials[self.by_id[c.get("id")]]), "ref " + c.get("id")
        else:
            it = c.get("type")
            if it in ("twosided", "mask", "bumpmap", "normalmap"):
                raise SceneError("%s(%s) is not supported: the nesting order is bumpmap(mask(twosided(%s(..))))" % (t, it, t))
            m = self._make_bsdf(c, allow_twosided=False)
        if "blend" in m:
            raise SceneError("%s(%s): blends of blends are not supported" % (t, it))
        if "coating" in m:
            raise SceneError("%s(%s): coated children are not supported" % (t, it))
        if m["type"] in (6, 7, 8):
            raise SceneError("%s(%s): dielectric, thindielectric and roughdielectric children are not supported" % (t, it))
        if m["type"] in (10, 11, 12):
            raise SceneError("%s(%s): roughdiffuse, difftrans and phong children are not supported" % (t, it))
        if m["type"] == 13:
            raise SceneError("%s(%s): a null child is not supported" % (t, it))
        if m["type"] == 1 or m.get("twosided") or "opacity" in m or "bump" in m or "normal_map" in m:
            raise SceneError("%s(%s) is not supported: the nesting order is bumpmap(mask(twosided(%s(..))))" % (t, it, t))
        return {k: v for k, v in m.items() if not k.startswith("_")}

    def _blended(self, elem, p, t):
        """the blended material's own record — diffuse, carrying nothing but the adapters that go around it — with the combinator under
        `blend` (bindings.Blend), its children as material dicts"""
        kids = [c for c in elem if c.tag == "bsdf" or (c.tag == "ref" and c.get("name") != "weight" and c.get("id") not in self.tex_by_id)]
        if len(kids) > 4:
            raise SceneError("%s: more than 4 nested bsdfs are not supported (found %d)" % (t, len(kids)))
        if t == "blendbsdf" and len(kids) != 2:
            raise SceneError("blendbsdf: BSDF count mismatch: expected two nested BSDF instances! (found %d)" % len(kids))
        b = dict(kind=t, children=tuple([self._blend_child(t, c) for c in kids]))
        if t == "blendbsdf":
            if _texture_on(elem, "weight"):
                w, ti = self._colour_or_texture(elem, "weight", 0.5, wrap=True)
                b["weight"] = float((f32(w[0]) + f32(w[1]) + f32(w[2])) * (f32(1.0) / f32(3)))  # Spectrum::average (spectrum.h:481-486)
                b["weight_texture"] = ti
            else:
                try:
                    b["weight"], b["weight_texture"] = float(f32(float(p.get("weight", 0.5)))), None
                except (TypeError, ValueError):
                    raise SceneError("blendbsdf: Could not parse the weight!")
            if not math.isfinite(b["weight"]) or b["weight"] < 0:
                raise SceneError("blendbsdf: weight must be finite and not negative")
        else:
            tokens = [w for w in re.split("[ ,;]+", str(p.get("weights", ""))) if w]
            if not tokens:
                raise SceneError("mixturebsdf: No weights were supplied!")
            try:
                weights = tuple(float(f32(float(w))) for w in tokens)
            except ValueError:
                raise SceneError("mixturebsdf: Could not parse the BSDF weights!")
            if len(weights) != len(kids):
                raise SceneError("mixturebsdf: BSDF count mismatch: %d bsdfs, but specified %d weights" % (len(kids), len(weights)))
            if not all(math.isfinite(w) and w >= 0 for w in weights):
                raise SceneError("mixturebsdf: weights must be finite and not negative")
            if not sum(weights) > 0:
                raise SceneError("mixturebsdf: The weights must sum to a value greater than zero!")
            b.update(weights=weights, ensure_energy_conservation=bool(p.get("ensureEnergyConservation", True)))
        return dict(type=0, reflectance=(0.5, 0.5, 0.5), blend=b)

    def _normal_adapter(self, elem, allow_twosided, key, label, strict_counts):
        """bumpmap (bumpmap.cpp:60-133: a displacement texture, `key` = bump) and normalmap (normalmap.cpp:47-106: an RGB normal map, normal_map): one nested BSDF +
        one texture, the outermost adapter.  `label` names the texture in the messages; strict_counts: a strict load refuses other child counts in the plug-in's words."""
        t, inner, maps = elem.get("type"), _nested_bsdfs(elem), [c for c in elem if self._is_texture(c)]
        if strict_counts and self.strict:  # normalmap.cpp:60-63, 91-96
            for bad, why in ((not inner, "A child BSDF instance is required"), (len(inner) > 1, "Only a single nested BSDF can be added!"),
                             (not maps, "A normal map texture must be specified"), (len(maps) > 1, "Only a single normal texture can be specified!")):
                if bad:
                    raise SceneError("normalmap: " + why)
        if len(inner) != 1 or (len(maps) != 1 and self.strict):
            return self._unsupported_bsdf(t)
        if len(maps) != 1:  # adapters around one nested BSDF: a lenient load renders the nested one
            self.warnings.append("bsdf %r dropped around its nested bsdf" % t)
            return self._make_bsdf(inner[0], allow_twosided)
        m = self._make_bsdf(inner[0], allow_twosided)
        try:
            for other, name in (("bump", "bumpmap"), ("normal_map", "normalmap")):
                if other in m:
                    raise SceneError("%s(%s(...)) is not supported" % (t, name))
            if m["type"] == 13:
                raise SceneError("%s(null) is not supported: the null BSDF has no shading frame to perturb" % t)
            if maps[0].tag == "texture" and maps[0].get("type") == "bitmap" and "gamma" not in _props(maps[0], self.sub):  # bumpmap.cpp:121-126, normalmap.cpp:97-100
                raise SceneError("When using a bitmap texture as a %s, please explicitly specify the 'gamma' parameter of the bitmap plugin" % label)
            return dict(m, **{key: self._bitmap_texture(maps[0], t)})
        except SceneError as e:
            if self.strict:
                raise
            self.warnings.append("%s dropped around its nested bsdf (%s)" % (label, e))
            return m

    def _make_bsdf(self, elem, allow_twosided=True):
        """<bsdf> → material dict (bindings.Material.from_dict), by the reader of its plug-in: _BSDF_READERS below.  allow_twosided = False inside a
        twosided, a coat or a blend: no twosided or mask goes there."""
        t, p = elem.get("type"), _props(elem, self.sub)
        reader = _BSDF_READERS.get(t)
        if reader is None or (t in ("twosided", "mask") and not allow_twosided):
            return self._unsupported_bsdf(t)
        return reader(self, elem, p, allow_twosided)

    def _intern(self, m):  # index of the material dict in `self.materials`, appended where no equal one is there yet, without its private `_` keys
        m ={k: v for k, v in m.items() if not k.startswith("_")}
        key = tuple(sorted((k, _freeze(v)) for k, v in m.items()))
        if key not in self.mat_index:
            self.mat_index[key] = len(self.materials)
            self.materials.append(m)
        return self.mat_index[key]

    def _read_integrator(self, root):
        """→ (the guided_path properties for ppg_create, the `field` integrators of a multichannel integrator (misc/multichannel.cpp))"""
        integ = root.find("integrator")
        if integ is None:
            raise SceneError("no <integrator>")
        fields = []
        if integ.get("type") == "multichannel":
            nested = [c for c in integ if c.tag == "integrator"]
            guided = [c for c in nested if c.get("type") == "guided_path"]
            other = [c.get("type") for c in nested if c.get("type") not in ("guided_path", "field")]
            if len(guided) != 1 or other:
                raise SceneError("a multichannel integrator must hold exactly one 'guided_path' and otherwise 'field' integrators only (found %s)"
                                 % (", ".join(repr(c.get("type")) for c in nested) or "none"))
            for c in nested:  # the `field` integrators (misc/field.cpp): (name, undefined rgb)
                if c.get("type") != "field":
                    continue
                name = _props(c, self.sub).get("field")
                if name == "shapeIndex":
                    raise SceneError("field integrator: 'shapeIndex' is not offered: shapes are flattened on loading, use 'primIndex'")
                if name not in FIELD_NAMES:
                    raise SceneError("field integrator: Invalid 'field' parameter. Must be one of 'position', 'relPosition', 'distance', 'geoNormal', "
                                     "'shNormal', 'primIndex', 'shapeIndex', or 'uv'! (got %r)" % (name,))
                undefined = np.zeros(3, f32)
                for u in c:
                    if u.get("name") == "undefined":
                        if u.tag == "float":
                            undefined = np.full(3, float(self.sub(u.get("value"))), f32)
                        elif u.tag in ("rgb", "srgb", "spectrum"):
                            undefined = np.asarray(spectrum.parse(u.tag, self.sub(u.get("value"))), f32)
                fields.append((name, tuple(float(v) for v in undefined)))
            integ = guided[0]
        if integ.get("type") != "guided_path":
            raise SceneError("integrator type %r is not supported: this path implements 'guided_path' only" % integ.get("type"))
        props = {}
        for k, v in _props(integ, self.sub).items():
            if k in GUIDED_PATH_PROPS:
                props[k] = GUIDED_PATH_PROPS[k](v)
            else:
                self.warnings.append("integrator property %r is not used by guided_path" % k)  # Mitsuba warns about unqueried properties, too
        return props, fields

    def _read_sensor(self, root, width, height):
        """<sensor> with its film and sampler → (the SceneDesc's camera, lens and rfilter, the info dict's width, height and sample_count)"""
        sensor = root.find("sensor")
        if sensor is None:
            raise SceneError("no <sensor>")
        stype = sensor.get("type")
        if stype not in ("perspective", "thinlens"):
            raise SceneError("sensor type %r is not supported (perspective, thinlens)" % stype)
        sp = _props(sensor, self.sub)
        film = sensor.find("film")
        fp = _props(film, self.sub) if film is not None else {}
        if film is not None and film.get("type") not in ("hdrfilm", "ldrfilm", None):
            raise SceneError("film type %r is not supported" % film.get("type"))
        rf = film.find("rfilter") if film is not None else None
        rfilter = parse_rfilter(rf, self.sub) if rf is not None else None
        if rf is None:
            self.warnings.append("no <rfilter>: Mitsuba would default to gaussian; the box filter is used")
        W = int(width or fp.get("width", 768)); H = int(height or fp.get("height", 576))
        if "fov" in sp and "focalLength" in sp:  # PerspectiveCamera::PerspectiveCamera, sensor.cpp:226-228
            raise SceneError("%s sensor: please specify either a focal length ('focalLength') or a field of view ('fov')" % stype)
        if "fov" in sp:
            fov, fov_axis = sp["fov"], str(sp.get("fovAxis", "x")).lower()
        else:
            fov, fov_axis = focal_length_fov(str(sp.get("focalLength", "50mm"))), "diagonal"
        tw = sensor.find("transform")
        c2w = _transform(tw, self.sub) if tw is not None else np.eye(4, dtype=f32)
        camera = perspective_camera_from_matrix(c2w, fov, fov_axis, sp.get("nearClip", 1e-2), sp.get("farClip", 1e4), W, H)
        lens = None
        if stype == "thinlens":  # ThinLens::ThinLens, thinlens.cpp:124-142; focusDistance defaults to farClip (sensor.cpp:162)
            if "apertureRadius" not in sp:
                raise SceneError("thinlens sensor without 'apertureRadius'")
            r = f32(sp["apertureRadius"])
            if r == 0:
                self.warnings.append("thinlens: can't have a zero aperture radius -- setting to 0.0001")
                r = f32(1e-4)
            focus = f32(sp.get("focusDistance", sp.get("farClip", 1e4)))
            if _has_scale(c2w):
                raise SceneError("thinlens sensor: scale factors in the camera-to-world transformation are not allowed")
            if not (np.isfinite(r) and r > 0 and np.isfinite(focus) and focus > 0):
                raise SceneError("thinlens sensor: apertureRadius and focusDistance must be finite and > 0 (got %r, %r)" % (float(r), float(focus)))
            lens = dict(aperture_radius=float(r), focus_distance=float(focus))
        camera_medium = 0
        for c in sensor:  # the medium the sensor lies in (Sensor::m_medium)
            if self._is_medium(c):
                index = self._medium_index(c, "the sensor's")
                camera_medium = 0 if index is None else 1 + index
        sampler = sensor.find("sampler")
        info = dict(width=W, height=H, sample_count=_props(sampler, self.sub).get("sampleCount") if sampler is not None else None)
        return dict(camera=camera, lens=lens, rfilter=rfilter, camera_medium=camera_medium), info

    # ---- participating media: <medium type="homogeneous"> with a nested <phase> (medium/homogeneous.cpp, medium.cpp, phase/isotropic.cpp, hg.cpp);
    # <medium type="heterogeneous"> further down
    def _make_medium(self, elem):
        """A <medium> element → its dict (bindings.Medium).  What cannot be rendered is refused by name."""
        t = elem.get("type")
        if t == "heterogeneous":
            return self._make_heterogeneous(elem)
        if t != "homogeneous":
            raise SceneError("medium type %r is not supported (homogeneous, heterogeneous)" % t)
        p = _props(elem, self.sub)
        stated = {c.get("name") for c in elem if c.tag in ("rgb", "srgb", "spectrum", "blackbody")}
        if "material" in p:
            raise SceneError("homogeneous medium: the 'material' presets (%r) are not supported: state sigmaA and sigmaS, or sigmaT and albedo" % p["material"])
        pair_as, pair_ta = {"sigmaA", "sigmaS"} & stated, {"sigmaT", "albedo"} & stated
        if pair_as and pair_ta:
            raise SceneError("homogeneous medium: please provide *either* sigmaA & sigmaS *or* sigmaT & albedo, but no other combinations!")  # materials.h:154-170
        if len(pair_as) != 2 and len(pair_ta) != 2:
            raise SceneError("homogeneous medium: state both sigmaA and sigmaS, or both sigmaT and albedo (Mitsuba fills what is missing from its "
                             "'material' preset table, which is not supported)")
        strategy = str(p.get("strategy", "balance"))
        if strategy == "maximum":
            raise SceneError("homogeneous medium: strategy 'maximum' is not supported (balance, single, manual)")
        if strategy not in ("balance", "single", "manual"):
            raise SceneError("homogeneous medium: Specified an unknown sampling strategy (%r)" % strategy)
        if p.get("monochromatic", False):
            raise SceneError("homogeneous medium: 'monochromatic' is not supported")
        colour = lambda name: tuple(float(v) for v in self._colour(elem, name, 0.0))  # noqa: E731
        m = dict(scale=float(p.get("scale", 1.0)), strategy=strategy)
        if len(pair_as) == 2:
            m.update(sigma_a=colour("sigmaA"), sigma_s=colour("sigmaS"))
        else:
            m.update(sigma_t=colour("sigmaT"), albedo=colour("albedo"))
        if strategy == "single" and "channel" in p:
            if int(p["channel"]) not in (0, 1, 2):
                raise SceneError("homogeneous medium: channel must be 0, 1 or 2")
            m["channel"] = int(p["channel"])
        if strategy == "manual":
            if "samplingDensity" not in p:
                raise SceneError("homogeneous medium: strategy 'manual' needs 'samplingDensity'")
            m["sampling_density"] = float(p["samplingDensity"])
        if "mediumSamplingWeight" in p and float(p["mediumSamplingWeight"]) != -1:
            m["sampling_weight"] = float(p["mediumSamplingWeight"])
        m.update(self._read_phase(elem, "homogeneous medium"))
        return m

    def _read_phase(self, elem, who):  # the nested <phase> of a <medium> → the dict's phase / g entries (none: Medium::configure instantiates `isotropic`)
        phases = [c for c in elem if c.tag == "phase"]
        if len(phases) > 1:
            raise SceneError("%s: more than one <phase>" % who)
        if not phases:
            return {}
        pt, pp = phases[0].get("type"), _props(phases[0], self.sub)
        if pt == "hg":
            g = float(pp.get("g", 0.8))  # hg.cpp:49-52
            if g >= 1 or g <= -1:
                raise SceneError("hg: The asymmetry parameter must lie in the interval (-1, 1)!")
            return dict(phase="hg", g=g)
        if pt != "isotropic":
            raise SceneError("phase function type %r is not supported (isotropic, hg)" % pt)
        return {}

    # ---- <medium type="heterogeneous"> (medium/heterogeneous.cpp, method = woodcock) over <volume type="constvolume|gridvolume">
    def _make_volume(self, elem, name):
        """A <volume name="density|albedo"> → its dict (bindings.Volume)"""
        t, want = elem.get("type"), (1 if name == "density" else 3)
        if t not in ("constvolume", "gridvolume"):
            raise SceneError("medium type 'heterogeneous': volume type %r (%s) is not supported (constvolume, gridvolume)" % (t, name))
        p = _props(elem, self.sub)  # (sendData is read by nobody)
        if t == "constvolume":
            values = [c for c in elem if c.get("name") == "value"]
            if len(values) != 1:
                raise SceneError("medium type 'heterogeneous': constvolume (%s) needs one 'value'" % name)
            if values[0].tag == "float":
                v = float(p["value"])
                return dict(value=v if want == 1 else (v, v, v))
            if values[0].tag in ("rgb", "srgb", "spectrum", "blackbody") and want == 3:
                return dict(value=tuple(float(x) for x in self._colour(elem, "value", 0.0)))
            raise SceneError("medium type 'heterogeneous': the constvolume for %s must hold a %s value (got <%s>)" % (name, "float" if want == 1 else "float or spectrum", values[0].tag))
        fn = p.get("filename")
        if not fn:
            raise SceneError("medium type 'heterogeneous': gridvolume (%s) without filename" % name)
        full = fn if os.path.isabs(fn) else os.path.join(self.base, fn)
        try:
            vol = read_vol(full)
        except (OSError, ValueError) as e:
            raise SceneError("medium type 'heterogeneous': gridvolume (%s) %r: %s" % (name, fn, e))
        if vol["data"].ndim == 4 and want == 1:
            raise SceneError("medium type 'heterogeneous': gridvolume %r has 3 channels: a density volume must have 1" % fn)  # Assert(m_channels == 1)
        if vol["data"].ndim == 3 and want == 3:
            raise SceneError("medium type 'heterogeneous': gridvolume %r has 1 channel: an albedo volume must have 3" % fn)  # Assert(m_channels == 3)
        to_world = None
        for c in elem:
            if c.tag == "transform" and c.get("name") == "toWorld":
                to_world = _transform(c, self.sub)
        lo, hi = (p["min"], p["max"]) if ("min" in p and "max" in p) else (vol["min"], vol["max"])  # gridvolume.cpp:104-110
        return dict(data=vol["data"], min=tuple(float(x) for x in lo), max=tuple(float(x) for x in hi), to_world=to_world)

    def _make_heterogeneous(self, elem):
        p = _props(elem, self.sub)
        stated = {c.get("name") for c in elem if c.tag in ("rgb", "srgb", "spectrum", "blackbody", "float")} & {"sigmaA", "sigmaS", "sigmaT", "albedo"}
        if stated:
            raise SceneError("medium type 'heterogeneous' is not supported (homogeneous media only) with %s: these belong to homogeneous media; give `density` and "
                             "`albedo` volumes" % " / ".join(repr(n) for n in sorted(stated)))
        method = str(p.get("method", "woodcock")).lower()
        if method == "simpson":
            raise SceneError("medium type 'heterogeneous': method 'simpson' is not supported (woodcock)")
        if method != "woodcock":
            raise SceneError("medium type 'heterogeneous': Unsupported integration method %r" % method)
        volumes = {}
        for c in elem:
            if c.tag != "volume":
                continue
            name = c.get("name")
            if name == "orientation":
                raise SceneError("medium type 'heterogeneous': an 'orientation' volume (anisotropic media) is not supported")
            if name not in ("density", "albedo"):
                raise SceneError("medium type 'heterogeneous': volume name %r is not supported (density, albedo)" % name)
            volumes[name] = self._make_volume(c, name)
        for name in ("density", "albedo"):
            if name not in volumes:
                raise SceneError("medium type 'heterogeneous': No %s specified!" % name)  # heterogeneous.cpp:229-232
        scale = float(p.get("scale", 1.0))
        m = dict(type="heterogeneous", density=volumes["density"], albedo=volumes["albedo"], scale=scale)  # (stepSize: tracking never reads it)
        m.update(self._read_phase(elem, "heterogeneous medium"))
        return m

    def _medium_index(self, elem, where):
        """The index in self.media of a <medium> or a <ref> to a top-level one; None where a lenient load has dropped it (with a warning)."""
        if elem.tag == "ref":
            rid = elem.get("id")
            if rid not in self.medium_by_id:
                raise SceneError("<ref id=%r>: no such medium" % rid)
            return self.medium_by_id[rid]
        try:
            m = self._make_medium(elem)
        except SceneError as e:
            if self.strict:
                raise
            self.warnings.append("medium dropped (%s): %s" % (where, e))
            return None
        self.media.append(m)
        if len(self.media) > 65535:
            raise SceneError("more than 65535 media")
        return len(self.media) - 1

    def _read_media(self, root):  # the top-level <medium id=...> elements → self.medium_by_id
        for m in root.findall("medium"):
            index = self._medium_index(m, "id %r" % m.get("id"))
            if m.get("id"):
                self.medium_by_id[m.get("id")] = index

    def _is_medium(self, c):  # whether the child element is a <medium>, or a <ref> to one (by its name or by its target)
        return c.tag == "medium" or (c.tag == "ref" and (c.get("name") in ("interior", "exterior") or c.get("id") in self.medium_by_id))

    def _shape_media_word(self, sh):  # the binding word of a <shape>: its interior / exterior media (bindings.media_word)
        from .bindings import media_word
        sides = dict(interior=None, exterior=None)
        for c in sh:
            if c.tag == "subsurface":
                if self.strict:
                    raise SceneError("subsurface plug-ins (<subsurface type=%r>) are not supported" % c.get("type"))
                self.warnings.append("subsurface %r on a shape dropped (not supported)" % c.get("type"))
            if not self._is_medium(c):
                continue
            name = c.get("name")
            if name not in sides:
                raise SceneError("a medium on a shape must be named 'interior' or 'exterior' (got %r)" % name)
            sides[name] = self._medium_index(c, "%s of a %s shape" % (name, sh.get("type")))
        return media_word(**sides)

    def _read_named_bsdfs(self, root):  # the <bsdf id=...> elements → self.by_id
        for b in root.findall("bsdf"):
            if b.get("id"):
                self.by_id[b.get("id")] = self._intern(self._make_bsdf(b))
        # an id may also sit on a NESTED bsdf (KITCHEN references the twosided element inside a bumpmap): every element with an id is a named
        # object in Mitsuba (scenehandler.cpp: namedObjects)
        for top in root.findall("bsdf"):
            for b in top.iter("bsdf"):
                if b is not top and b.get("id") and b.get("id") not in self.by_id:
                    self.by_id[b.get("id")] = self._intern(self._make_bsdf(b))

    def _rotation(self, em, what):  # the 3x3 of an environment emitter's toWorld, which must be a rotation
        tw = em.find("transform")
        R = (_transform(tw, self.sub) if tw is not None else np.eye(4, dtype=f32))[:3, :3].astype(f32)
        if not np.allclose(R @ R.T, np.eye(3), atol=1e-4):
            raise SceneError("%s: toWorld must be a rotation" % what)
        return [float(v) for v in R.reshape(-1)]

    def _read_sunsky(self, em):
        """SunSkyEmitter (sunsky.cpp:100-235) bakes sun + sky into a radiance map and instantiates `envmap` on it: same bake here (ppg_host/sunsky.py);
        the Hosek-Wilkie / Preetham tables are read from the operator's Mitsuba source tree.  None where a lenient load finds no such tree."""
        from . import sunsky
        ddir = self.data_dir or os.environ.get("PPG_MITSUBA_DATA")
        src = self.mitsuba_src or os.environ.get("PPG_MITSUBA_SRC") or (os.path.dirname(os.path.abspath(ddir)) if ddir else None)
        if not src or not os.path.exists(os.path.join(src, "src", "emitters", "sunsky", "skymodeldata.h")):
            if self.strict:
                raise SceneError("sunsky: the sky model's coefficient tables (src/emitters/sunsky/skymodeldata.h, sunmodel.h) come with Mitsuba's "
                                 "source tree: pass mitsuba_src / --data-dir <tree>/data / PPG_MITSUBA_SRC")
            self.warnings.append("emitter 'sunsky' skipped (no Mitsuba source tree for the sky model's tables)")
            return None
        ep = _props(em, self.sub)
        for c in em:
            if c.get("name") == "albedo" and c.tag in ("rgb", "srgb", "spectrum"):
                ep["albedo"] = [float(v) for v in spectrum.parse(c.tag, self.sub(c.get("value")))]
        try:
            rgb, _ = sunsky.bake(ep, src)
        except (ValueError, NotImplementedError) as e:
            raise SceneError("sunsky: %s" % e)
        return dict(rgb=rgb, scale=1.0, to_world=self._rotation(em, "sunsky"))

    def _read_emitters(self, root):  # the top-level <emitter>s → SceneDesc's environment, envmap, delta_emitters; only the first environment emitter counts
        environment = envmap = None
        delta_emitters = []
        for em in root.findall("emitter"):
            t = em.get("type")
            if any(self._is_medium(c) for c in em):
                if self.strict:
                    raise SceneError("a <medium> inside an emitter (%r) is not supported: media are attached to shapes and to the sensor" % t)
                self.warnings.append("medium inside emitter %r dropped (not supported)" % t)
            if t in ("point", "spot", "directional"):
                delta_emitters.append(parse_delta_emitter(em, self))
            elif t == "constant" and environment is None and envmap is None:
                environment = tuple(float(v) for v in self._colour(em, "radiance", 1.0))
            elif t == "envmap" and environment is None and envmap is None:  # EnvironmentMap::EnvironmentMap, envmap.cpp:100-190
                from . import imageio
                ep = _props(em, self.sub)
                fn = ep.get("filename")
                if not fn:
                    raise SceneError("envmap emitter without filename")
                full = fn if os.path.isabs(fn) else os.path.join(self.base, fn)
                if not os.path.exists(full):
                    raise SceneError("envmap: file '%s' not found" % full)
                try:
                    rgb = imageio.read_image(full)
                except (ValueError, AssertionError) as e:
                    raise SceneError("envmap: %s" % e)
                envmap = dict(rgb=rgb, scale=float(ep.get("scale", 1.0)), to_world=self._rotation(em, "envmap"))
            elif t == "sunsky" and environment is None and envmap is None:
                envmap = self._read_sunsky(em)
            elif not self.strict:
                self.warnings.append("emitter %r skipped (not supported)" % t)
            else:
                raise SceneError("emitter type %r is not supported (area emitters on shapes, `point`, `spot` and `directional` emitters, and one "
                                 "`constant`, `envmap` or `sunsky` environment emitter; SURVEY.md §8 f2)" % t)
        return dict(environment=environment, envmap=envmap, delta_emitters=delta_emitters)

    def _mesh_file(self, t, sprops):
        """The file of an obj / ply / serialized shape, or None where a lenient load skips a shape without one.  (obj.cpp tests its properties before it opens the file.)"""
        fn, label = sprops.get("filename"), {"obj": "Wavefront OBJ file", "ply": "PLY file", "serialized": "serialized mesh file"}[t]
        if not fn:
            raise SceneError("%s shape without filename" % t)
        if t == "obj" and "shapeIndex" in sprops:
            raise SceneError("obj: shapeIndex is not supported")
        both = "maxSmoothAngle" in sprops and sprops.get("faceNormals", False)
        if t == "obj" and both:
            raise SceneError("The properties 'maxSmoothAngle' and 'faceNormals' can't be specified at the same time!")  # obj.cpp:337-339
        full = fn if os.path.isabs(fn) else os.path.join(self.base, fn)
        if not os.path.exists(full):
            if self.strict:
                raise SceneError("%s '%s' not found%s" % (label, full, "!" if t == "obj" else ""))  # obj.cpp:230
            self.warnings.append("shape skipped: %s '%s' not found" % (label, full))
            return None
        if both:
            raise SceneError("The properties 'maxSmoothAngle' and 'faceNormals' can't be specified at the same time!")
        return full

    def _shape_geometry(self, sh):  # (the triangle meshes of a <shape>, its analytic record or None); None where a lenient load skips the shape
        t = sh.get("type")
        sprops = _props(sh, self.sub)
        tw = sh.find("transform")
        m = _transform(tw, self.sub) if tw is not None else np.eye(4, dtype=f32)
        face_normals, flip_normals = bool(sprops.get("faceNormals", False)), bool(sprops.get("flipNormals", False))
        if t in ("obj", "ply", "serialized"):
            full = self._mesh_file(t, sprops)
            if full is None:
                return None
            if t == "obj":
                return load_obj(full, m, face_normals, flip_normals, bool(sprops.get("flipTexCoords", True)), bool(sprops.get("collapse", False)),
                                sprops.get("maxSmoothAngle")), None
            if t == "ply":
                return [load_ply(full, m, face_normals, flip_normals, sprops.get("maxSmoothAngle"))], None
            return [load_serialized(full, m, int(sprops.get("shapeIndex", 0)), face_normals, flip_normals, sprops.get("maxSmoothAngle"))], None
        if t == "rectangle":
            return [rectangle_mesh(m, flip_normals)], None
        if t == "cube":
            return [cube_mesh(m, flip_normals)], None
        if t == "sphere":  # Sphere::Sphere, sphere.cpp:108-131: the scale of toWorld goes into the radius, the rest stays a rotation
            c = np.asarray(sprops.get("center", (0.0, 0.0, 0.0)), f32)
            o2w = _translate(*[float(v) for v in c])
            radius = f32(sprops.get("radius", 1.0))
            if tw is not None:
                scale = np.sqrt(np.sum(m[:3, 0] * m[:3, 0], dtype=f32), dtype=f32)  # objectToWorld(Vector(1, 0, 0)).length()
                o2w = (m @ _scale(*[float(f32(1) / scale)] * 3)).astype(f32) @ o2w
                o2w = o2w.astype(f32)
                radius = f32(radius * scale)
            if not radius > 0:
                raise SceneError("Cannot create spheres of radius <= 0")
            return [], dict(center=tuple(float(v) for v in o2w[:3, 3]), radius=float(radius), to_world=[float(v) for v in o2w[:3, :3].reshape(-1)],
                            flip_normals=flip_normals)
        if t == "disk":
            return [], disk_shape(_transform64(tw, self.sub) if tw is not None else np.eye(4), flip_normals)
        if t == "cylinder":
            # (An element that states nothing — no p0, p1, radius or toWorld — is refused, although Mitsuba would make the unit cylinder of
            # it: `<shape type="cylinder"/>` is what the suite has always used as its example of a shape this loader names and refuses
            # (tests/test_mitsuba_xml.py, tests/test_cpp_host.py), and that pin stays.  Every cylinder of a real scene states its geometry.)
            if tw is None and not any(k in sprops for k in ("p0", "p1", "radius")):
                raise SceneError("cylinder: none of p0, p1, radius, toWorld is given; state the cylinder's geometry (Mitsuba's defaults — the "
                                 "unit cylinder from the origin along z — are not assumed here)")
            return [], cylinder_shape(_transform64(tw, self.sub) if tw is not None else None, sprops.get("p0", (0.0, 0.0, 0.0)), sprops.get("p1", (0.0, 0.0, 1.0)),
                                      sprops.get("radius", 1.0), flip_normals)
        raise SceneError("shape type %r is not supported (obj, ply, serialized, rectangle, cube, sphere, disk, cylinder)" % t)

    def _attach(self, sh, meshes, analytic, out):
        """Give a <shape>'s geometry its material (nested <bsdf> or <ref id>) and area emitter and append it to `out`; refuses what analytic shapes cannot carry"""
        t, e, mat, em = sh.get("type"), sh.find("emitter"), None, -1
        word = self._shape_media_word(sh)
        for c in sh:
            if c.tag == "bsdf":
                mat = self._intern(self._make_bsdf(c))
            elif c.tag == "ref" and not self._is_medium(c):
                rid = c.get("id")
                if rid not in self.by_id:
                    raise SceneError("<ref id=%r>: no such bsdf" % rid)
                mat = self.by_id[rid]
        if mat is None:  # Shape::configure (shape.cpp:48-72): all-absorbing under an emitter, otherwise a 0.5 Lambertian "for convenience"
            mat = self._intern(dict(type=0, reflectance=(0.0, 0.0, 0.0) if e is not None else (0.5, 0.5, 0.5)))
        if e is not None:
            if e.get("type") != "area":
                raise SceneError("emitter type %r on a shape is not supported (area only)" % e.get("type"))
            if len(meshes) > 1:
                raise SceneError("Cannot attach an emitter to an OBJ file containing multiple objects!")  # obj.cpp:757-759
            if t == "obj" and not meshes:
                return
            em = len(out["emitters"])
            out["emitters"].append(dict(radiance=tuple(float(v) for v in self._colour(e, "radiance", 1.0))))
        out["meshes"] += [(dict(mesh, media_word=word), mat, em) for mesh in meshes]
        if analytic is None:
            return
        material = self.materials[mat]
        if "blend" in material and _reads_bitmap(material):
            raise SceneError("%s: %s: textured BSDFs are only supported on triangle meshes (not on spheres, disks or cylinders)" % (t, material["blend"]["kind"]))
        if material.get("type") == 13:
            raise SceneError("%s: the null BSDF is only supported on triangle meshes (not on spheres, disks or cylinders)" % t)
        out["sphere_media" if t == "sphere" else "shape_media"].append(word)
        if t == "sphere":
            out["spheres"].append(dict(analytic, material=mat, emitter=em))
        else:
            if any(material.get(k) is not None for k in TEXTURE_KEYS):
                raise SceneError("%s: textured BSDFs are only supported on triangle meshes (not on spheres, disks or cylinders)" % t)
            out["shapes"].append(dict(analytic, material=mat, emitter=em))

    def _read_shapes(self, root):  # the <shape>s → meshes [(mesh dict, material index, emitter index or -1)], SceneDesc's emitters, spheres and shapes
        out = dict(meshes=[], emitters=[], spheres=[], shapes=[], sphere_media=[], shape_media=[])
        for sh in root.findall("shape"):
            geometry = self._shape_geometry(sh)
            if geometry is not None:
                self._attach(sh, *geometry, out)
        if not out["meshes"] and not out["spheres"] and not out["shapes"]:
            raise SceneError("scene without shapes")
        for k in ("sphere_media", "shape_media"):  # (None: no transitions among them)
            out[k] = np.asarray(out[k], np.uint32) if any(out[k]) else None
        return out.pop("meshes"), out

    def _flatten(self, meshes):
        """The scene's meshes as one vertex and one triangle list → the SceneDesc's positions, indices, tri_material, tri_emitter, normals, texcoords.
        One vertex-normal array serves the whole scene: a faceNormals mesh living next to smooth ones gets its vertices un-shared and its face
        normals written out (same shading frame as "no normals": skdtree.h:388-401).  Texture coordinates only matter on meshes whose BSDF reads a
        bitmap or is anisotropic; the others get NaN rows (= none).  (A blended material asks for what its weight or any of its children asks for.)"""
        wants_uvs = lambda mat: _reads_bitmap(self.materials[mat]) or _anisotropic(self.materials[mat])  # noqa: E731
        any_normals = any(m["normals"] is not None for m, _, _ in meshes)
        any_uvs = any(m.get("uvs") is not None and wants_uvs(mat) for m, mat, _ in meshes)
        # (each list starts with an empty array of its type: a scene of analytic shapes only has no mesh to concatenate)
        pos, idx, tmat, tem = [np.zeros((0, 3), f32)], [np.zeros((0, 3), np.uint32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.int32)]
        nrm, uvl, nv, tmed = [], [], 0, [np.zeros(0, np.uint32)]
        for mesh, mat, em in meshes:
            p, i, n = mesh["positions"], mesh["indices"], mesh["normals"]
            uv = mesh.get("uvs") if wants_uvs(mat) else None
            if uv is None and _anisotropic(self.materials[mat]):  # trimesh.cpp:686-691
                raise SceneError('"%s": computeUVTangents(): texture coordinates are required to generate tangent vectors. If you want to render with an '
                                 'anisotropic material, please make sure that all associated shapes have valid texture coordinates.%s'
                                 % (mesh.get("name", "mesh"), " (This loader's rectangle and cube carry none.)" if mesh.get("name") in ("rectangle", "cube") else ""))
            if any_normals and n is None:
                if uv is not None:
                    uv = uv[i.reshape(-1)]
                p = p[i.reshape(-1)]
                a, b = p[1::3] - p[0::3], p[2::3] - p[0::3]
                fnrm = np.cross(a, b).astype(f32)
                ln = np.sqrt(np.sum(fnrm * fnrm, 1)).astype(f32)
                fnrm[ln != 0] = fnrm[ln != 0] / ln[ln != 0, None]
                n = np.repeat(fnrm, 3, 0)
                i = np.arange(p.shape[0], dtype=np.uint32).reshape(-1, 3)
            T = i.shape[0]
            pos.append(p); idx.append(i + np.uint32(nv)); nrm.append(n)
            uvl.append(uv.astype(f32) if uv is not None else np.full((p.shape[0], 2), np.nan, f32))
            nv += p.shape[0]
            tmat.append(np.full(T, mat, np.uint32)); tem.append(np.full(T, em, np.int32)); tmed.append(np.full(T, mesh.get("media_word", 0), np.uint32))
        tri_media = np.concatenate(tmed)
        return dict(tri_media=tri_media if tri_media.any() else None, positions=np.concatenate(pos).astype(f32), indices=np.concatenate(idx).astype(np.uint32), tri_material=np.concatenate(tmat),
                    tri_emitter=np.concatenate(tem), normals=np.concatenate(nrm).astype(f32) if any_normals else None,
                    texcoords=np.concatenate(uvl).astype(f32) if any_uvs else None)

    def _assemble(self, meshes, **fields):  # the SceneDesc of the reader's tables, the flattened meshes and what the element readers returned
        from .bindings import expand_blends  # (children of blended materials join the list, behind everything a shape refers to)
        return SceneDesc(materials=expand_blends(self.materials), textures=self.textures, media=self.media, rtrans=np.stack(self.rt_slices).astype(f32) if self.rt_slices else None,
                         **self._flatten(meshes), **fields)


_BSDF_READERS = {  # plug-in → its reader (the reader object, the <bsdf> element, its simple properties, allow_twosided) → material dict
    "diffuse": lambda rd, elem, p, allow_twosided: rd._textured(elem, dict(type=0), "reflectance", 0.5),
    "null": lambda rd, elem, p, allow_twosided: dict(type=13),  # null.cpp:36-80: no parameters
    "bumpmap": lambda rd, elem, p, allow_twosided: rd._normal_adapter(elem, allow_twosided, "bump", "bump map", strict_counts=False),
    "normalmap": lambda rd, elem, p, allow_twosided: rd._normal_adapter(elem, allow_twosided, "normal_map", "normal map", strict_counts=True),
    "roughdiffuse": _Reader._read_roughdiffuse, "difftrans": _Reader._read_difftrans, "phong": _Reader._read_phong,
    "conductor": _Reader._read_conductor, "roughconductor": _Reader._read_conductor, "plastic": _Reader._read_plastic, "roughplastic": _Reader._read_roughplastic,
    "dielectric": _Reader._read_dielectric, "thindielectric": _Reader._read_dielectric, "roughdielectric": _Reader._read_roughdielectric,
    "twosided": _Reader._read_twosided, "mask": _Reader._read_mask, "coating": _Reader._read_coating, "roughcoating": _Reader._read_coating,
    "blendbsdf": _Reader._read_blend, "mixturebsdf": _Reader._read_blend,
}


VOL_ENCODINGS = {1: "float32", 2: "float16", 3: "uint8", 4: "quantized directions"}


def read_vol(path):
    """Mitsuba's .vol container (gridvolume.cpp:64-81: 'VOL', version 3, encoding, x / y / z cells, channels, the data's box; 48 bytes, little
    endian) → dict(data=float32 [z, y, x] or [z, y, x, 3], min, max, encoding).  uint8 texels become float32 as i / 255.0f, the reference's
    m_densityMap.  float16 and quantized directions are refused (the reference's float lookup answers 0 for them); so is a bad header."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 48 or raw[:3] != b"VOL":
        raise ValueError("bad header: not a .vol file (no 'VOL' signature in 48 header bytes)")
    if raw[3] != 3:
        raise ValueError("bad header: file format version %d (3 is supported)" % raw[3])
    enc, rx, ry, rz, ch = (int(v) for v in np.frombuffer(raw, "<i4", 5, 4))
    box = np.frombuffer(raw, "<f4", 6, 24)
    if enc not in VOL_ENCODINGS:
        raise ValueError("bad header: unknown encoding %d" % enc)
    if enc in (2, 4):
        raise ValueError("encoding %s is not supported (float32, uint8)" % VOL_ENCODINGS[enc])
    if min(rx, ry, rz) < 1 or ch not in (1, 3):
        raise ValueError("bad header: %d x %d x %d cells, %d channels (1 or 3 are supported)" % (rx, ry, rz, ch))
    n = rx * ry * rz * ch
    size = n * (4 if enc == 1 else 1)
    if len(raw) < 48 + size:
        raise ValueError("bad header: the file holds %d data bytes, %d x %d x %d x %d %s texels need %d" % (len(raw) - 48, rx, ry, rz, ch, VOL_ENCODINGS[enc], size))
    if enc == 1:
        data = np.frombuffer(raw, "<f4", n, 48).astype(f32)
    else:
        data = (np.arange(256, dtype=f32) / f32(255.0))[np.frombuffer(raw, np.uint8, n, 48)]
    data = data.reshape((rz, ry, rx) if ch == 1 else (rz, ry, rx, ch))
    return dict(data=np.ascontiguousarray(data), min=tuple(float(v) for v in box[:3]), max=tuple(float(v) for v in box[3:]), encoding=VOL_ENCODINGS[enc])


def write_vol(path, data, min, max, encoding="float32"):  # noqa: A002 (Mitsuba's names)
    """Write `data` ([z, y, x] or [z, y, x, 3]) as a .vol file; encoding "float32" or "uint8" (texels rounded to i / 255)."""
    data = np.asarray(data)
    if data.ndim not in (3, 4) or (data.ndim == 4 and data.shape[3] not in (1, 3)):
        raise ValueError("write_vol: data must be [z, y, x] or [z, y, x, 3]")
    if encoding not in ("float32", "uint8"):
        raise ValueError("write_vol: encoding %r is not supported (float32, uint8)" % (encoding,))
    rz, ry, rx = data.shape[:3]
    ch = 1 if data.ndim == 3 else data.shape[3]
    head = b"VOL\x03" + np.asarray([1 if encoding == "float32" else 3, rx, ry, rz, ch], "<i4").tobytes() + np.asarray(list(min) + list(max), "<f4").tobytes()
    if encoding == "float32":
        body = np.ascontiguousarray(data, "<f4").tobytes()
    elif data.dtype == np.uint8:
        body = np.ascontiguousarray(data).tobytes()
    else:
        body = np.clip(np.rint(np.asarray(data, np.float64) * 255.0), 0, 255).astype(np.uint8).tobytes()
    with open(path, "wb") as f:
        f.write(head + body)


def load_scene(path, defines=None, strict=True, width=None, height=None, data_dir=None, mitsuba_src=None):
    """Parse `path` → (SceneDesc, integrator properties for ppg_create, info dict).

    defines: {"name": "value"} like `mitsuba -D name=value`; width/height override the film size; data_dir: the `data` directory of a Mitsuba tree
    (default $PPG_MITSUBA_DATA), for data/microfacet/*.dat and data/ior/*.spd; mitsuba_src: the tree (default $PPG_MITSUBA_SRC, or data_dir's parent), for `sunsky`."""
    root = ET.parse(path).getroot()
    if root.tag != "scene":
        raise SceneError("%s: root element is <%s>, expected <scene>" % (path, root.tag))
    rd = _Reader(root, path, defines, strict, data_dir, mitsuba_src)
    props, fields = rd._read_integrator(root)
    rd._read_media(root)
    sensor, info = rd._read_sensor(root, width, height)
    rd._read_named_bsdfs(root)
    lights = rd._read_emitters(root)
    meshes, shapes = rd._read_shapes(root)
    desc = rd._assemble(meshes, **sensor, **lights, **shapes)
    if desc.delta_emitters and str(props.get("nee", "never")) != "always":
        rd.warnings.append("point / spot / directional emitters are reached by next-event estimation only: with nee = %s they contribute nothing in "
                           "every iteration that runs without it (as in Mitsuba)" % props.get("nee", "never"))
    info.update(fields=fields, warnings=rd.warnings)
    return desc, props, info


# ---------------------------------------------------------------------------------------------- writer
def save_scene_xml(desc, props, directory, name="scene"):
    """Write `desc` as <directory>/<name>.xml + meshes/*.obj in the subset above (one OBJ per material / emitter group),
    so that a procedural scene can be rendered by the reference itself — or read back by load_scene().  Returns the XML path."""
    if getattr(desc, "media", None):
        raise NotImplementedError("save_scene_xml: participating media (SceneDesc.media) are not written")
    os.makedirs(os.path.join(directory, "meshes"), exist_ok=True)
    cam = desc.camera
    c = lambda v: ", ".join(repr(float(x)) for x in v)  # noqa: E731
    out = ['<?xml version="1.0" encoding="utf-8"?>', '<scene version="0.5.0">', '\t<integrator type="guided_path">']
    for k, v in props.items():
        if k not in GUIDED_PATH_PROPS:
            continue
        t = GUIDED_PATH_PROPS[k]
        if k in ("strictNormals", "hideEmitters", "dumpSDTree"):
            out.append('\t\t<boolean name="%s" value="%s"/>' % (k, "true" if v else "false"))
        elif t is int:
            out.append('\t\t<integer name="%s" value="%d"/>' % (k, int(v)))
        elif t is float:
            out.append('\t\t<float name="%s" value="%r"/>' % (k, float(v)))
        else:
            out.append('\t\t<string name="%s" value="%s"/>' % (k, v))
    lens = getattr(desc, "lens", None)
    out += ['\t</integrator>', '\t<sensor type="%s">' % ("perspective" if lens is None else "thinlens"),
            '\t\t<string name="fovAxis" value="%s"/>' % cam.get("fov_axis", "x"), '\t\t<float name="fov" value="%r"/>' % float(cam["fov"]),
            '\t\t<float name="nearClip" value="%r"/>' % float(cam["near_clip"]), '\t\t<float name="farClip" value="%r"/>' % float(cam["far_clip"]),
            '\t\t<transform name="toWorld">', '\t\t\t<matrix value="%s"/>' % " ".join(repr(float(x)) for x in np.asarray(cam["camera_to_world"]).reshape(-1)),
            '\t\t</transform>'] + ([] if lens is None else [
            '\t\t<float name="apertureRadius" value="%r"/>' % float(lens["aperture_radius"]),
            '\t\t<float name="focusDistance" value="%r"/>' % float(lens["focus_distance"])]) + ['\t\t<sampler type="independent"/>', '\t\t<film type="hdrfilm">',
            '\t\t\t<integer name="width" value="%d"/>' % cam["width"], '\t\t\t<integer name="height" value="%d"/>' % cam["height"],
            '\t\t\t<boolean name="banner" value="false"/>', '\t\t\t<rfilter type="box"/>', '\t\t</film>', '\t</sensor>']
    from .bindings import Blend, Coating, Material, Microfacet, expand_blends
    mats = expand_blends(desc.materials)

    def leaf(m):
        """(the <bsdf> element of a material without its two-sided / mask adapters — "%s" takes its id attribute —, its type, its record)"""
        t = m.get("type", 0)
        t = Material.BSDF[t] if isinstance(t, str) else int(t)
        M = Material.from_dict(m)
        G = Microfacet.from_dict(m)  # a general entry is written as alphaU / alphaV (also when they are equal), phong, sampleVisible
        distr = "phong" if G.general and G.distribution == 1 else ("beckmann" if M.flags & 8 else "ggx")
        rough = '<string name="distribution" value="%s"/>' % distr
        if G.general:
            rough += '<float name="alphaU" value="%r"/><float name="alphaV" value="%r"/>' % (float(M.alpha), float(G.alpha_v))
            rough += '<boolean name="sampleVisible" value="false"/>' if G.sample_all else ""
        else:
            rough += '<float name="alpha" value="%r"/>' % float(M.alpha)
        R, S, E, K = (c(getattr(M, n)) for n in ("reflectance", "specular", "eta", "k"))
        one = '<float name="extIOR" value="1.0"/><float name="intIOR" value="%r"/>' % float(M.eta[0])
        body = {
            0: '<bsdf type="diffuse"%%s><rgb name="reflectance" value="%s"/></bsdf>' % R,
            1: '<bsdf type="diffuse"%%s><rgb name="reflectance" value="%s"/></bsdf>' % R,
            2: '<bsdf type="conductor"%%s><string name="material" value="none"/><rgb name="specularReflectance" value="%s"/></bsdf>' % R,
            3: '<bsdf type="conductor"%%s><float name="extEta" value="1.0"/><rgb name="eta" value="%s"/><rgb name="k" value="%s"/>'
               '<rgb name="specularReflectance" value="%s"/></bsdf>' % (E, K, R),
            4: '<bsdf type="roughconductor"%%s>%s<float name="extEta" value="1.0"/>'
               '<rgb name="eta" value="%s"/><rgb name="k" value="%s"/><rgb name="specularReflectance" value="%s"/></bsdf>'
               % (rough, E, K, R),
            5: '<bsdf type="plastic"%%s>%s<rgb name="diffuseReflectance" value="%s"/><rgb name="specularReflectance" value="%s"/>'
               '<boolean name="nonlinear" value="%s"/></bsdf>' % (one, R, S, "true" if M.flags & 2 else "false"),
            6: '<bsdf type="dielectric"%%s>%s<rgb name="specularReflectance" value="%s"/><rgb name="specularTransmittance" value="%s"/></bsdf>' % (one, R, S),
            7: '<bsdf type="thindielectric"%%s>%s<rgb name="specularReflectance" value="%s"/><rgb name="specularTransmittance" value="%s"/></bsdf>' % (one, R, S),
            8: '<bsdf type="roughdielectric"%%s>%s%s'
               '<rgb name="specularReflectance" value="%s"/><rgb name="specularTransmittance" value="%s"/></bsdf>'
               % (rough, one, R, S),
            9: '<bsdf type="roughplastic"%%s>%s%s'
               '<rgb name="diffuseReflectance" value="%s"/><rgb name="specularReflectance" value="%s"/><boolean name="nonlinear" value="%s"/></bsdf>'
               % (rough, one, R, S, "true" if M.flags & 2 else "false"),
            # (the values are the configured ones: whatever ensureEnergyConservation made of them when the scene was read)
            10: '<bsdf type="roughdiffuse"%%s><rgb name="reflectance" value="%s"/><float name="alpha" value="%r"/><boolean name="useFastApprox" value="%s"/>'
                '<boolean name="ensureEnergyConservation" value="false"/></bsdf>' % (R, float(M.alpha), "true" if M.flags & 16 else "false"),
            11: '<bsdf type="difftrans"%%s><rgb name="transmittance" value="%s"/><boolean name="ensureEnergyConservation" value="false"/></bsdf>' % R,
            12: '<bsdf type="phong"%%s><rgb name="diffuseReflectance" value="%s"/><rgb name="specularReflectance" value="%s"/><float name="exponent" value="%r"/>'
                '<boolean name="ensureEnergyConservation" value="false"/></bsdf>' % (R, S, float(M.alpha)),
            13: '<bsdf type="null"%s/>',
        }[t]
        K = Coating.from_dict(m)  # a coating / roughcoating goes around the leaf, inside the other adapters
        if K.kind:
            coat = '<float name="extIOR" value="1.0"/><float name="intIOR" value="%r"/><float name="thickness" value="%r"/>' % (float(K.eta), float(K.thickness))
            coat += '<rgb name="sigmaA" value="%s"/><rgb name="specularReflectance" value="%s"/>' % (c(K.sigma_a), c(K.specular))
            if K.kind == 2:
                coat += '<float name="alpha" value="%r"/><string name="distribution" value="%s"/>' % (float(K.alpha), ("beckmann", "ggx", "phong")[K.distribution])
                coat += '<boolean name="sampleVisible" value="false"/>' if K.sample_all else ""
            body = '<bsdf type="%s"%%s>%s%s</bsdf>' % ("coating" if K.kind == 1 else "roughcoating", coat, body % "")
        return body, t, M

    def normal_map_element(k):
        """the <texture type="bitmap"> of a normalmap adapter: texture k of the description written out as a PFM file — the texels as they
        are, a `scale` texture the loader folded into them included — with the lookup's parameters"""
        from . import imageio
        tex = desc.textures[k]
        fn = "%s_tex%d.pfm" % (name, k)
        imageio.write_pfm(os.path.join(directory, fn), np.ascontiguousarray(tex["rgb"], np.float32))
        wrap = lambda w: w if isinstance(w, str) else ("repeat", "mirror", "clamp", "zero", "one")[int(w)]  # noqa: E731
        su, sv = tex.get("uv_scale", (1.0, 1.0))
        ou, ov = tex.get("uv_offset", (0.0, 0.0))
        return ('<texture type="bitmap"><string name="filename" value="%s"/><float name="gamma" value="1.0"/><string name="wrapModeU" value="%s"/>'
                '<string name="wrapModeV" value="%s"/><string name="filterType" value="%s"/><float name="uscale" value="%r"/><float name="vscale" value="%r"/>'
                '<float name="uoffset" value="%r"/><float name="voffset" value="%r"/></texture>'
                % (fn, wrap(tex.get("wrap_u", "repeat")), wrap(tex.get("wrap_v", "repeat")), "nearest" if tex.get("nearest") else "bilinear",
                   float(np.float32(su)), float(np.float32(sv)), float(np.float32(ou)), float(np.float32(ov))))

    for i, m in enumerate(mats):
        body, t, M = leaf(m)
        B = Blend.from_dict(m)  # a blendbsdf / mixturebsdf stands where the leaf would, its children nested in it (a bitmap weight as its constant)
        if B.kind:
            kids = "".join(leaf(mats[B.child[k]])[0] % "" for k in range(B.n))
            if B.kind == 1:
                body = '<bsdf type="blendbsdf"%%s><float name="weight" value="%r"/>%s</bsdf>' % (float(B.weight[0]), kids)
            else:
                body = '<bsdf type="mixturebsdf"%%s><string name="weights" value="%s"/><boolean name="ensureEnergyConservation" value="%s"/>%s</bsdf>' % (
                    ", ".join(repr(float(B.weight[k])) for k in range(B.n)), "true" if B.ensure_energy_conservation else "false", kids)
        twos = t == 1 or (M.flags & 1 and t not in (6, 7, 8, 11, 13))
        ident = ' id="mat%d"' % i
        nmap = (M.texture >> 16) - 1 if M.flags & Material.NORMALMAP and M.texture >> 16 else None  # a normalmap adapter goes around everything else
        own = "" if nmap is not None else ident
        if M.flags & 4:
            inner = ('<bsdf type="twosided">%s</bsdf>' % (body % "")) if twos else body % ""
            element = '<bsdf type="mask"%s><rgb name="opacity" value="%s"/>%s</bsdf>' % (own, c(M.opacity), inner)
        elif twos:
            element = '<bsdf type="twosided"%s>%s</bsdf>' % (own, body % "")
        else:
            element = body % own
        if nmap is not None:
            element = '<bsdf type="normalmap"%s>%s%s</bsdf>' % (ident, normal_map_element(nmap), element)
        out.append('\t' + element)
    tm, te = np.asarray(desc.tri_material), np.asarray(desc.tri_emitter)
    idx, pos = np.asarray(desc.indices), np.asarray(desc.positions)
    groups = sorted({(int(a), int(b)) for a, b in zip(tm, te)}, key=lambda g: (g[1] < 0, g[1], g[0]))  # emitters first, in emitter order
    # shapes in emitter order (the loader numbers emitters in shape order), shapes without an emitter last
    shapes = [("mesh", g) for g in groups] + [("sphere", sp) for sp in (getattr(desc, "spheres", None) or [])]
    shapes += [("shape", sh) for sh in (getattr(desc, "shapes", None) or [])]
    em_of = lambda rec: rec[1][1] if rec[0] == "mesh" else int(rec[1].get("emitter", -1))  # noqa: E731
    # (a disk or cylinder without an emitter stays behind the emitting one that precedes it in desc.shapes: the list comes back in its order)
    order, prev = {}, -1
    for k, sh in enumerate(getattr(desc, "shapes", None) or []):
        prev = int(sh.get("emitter", -1)) if int(sh.get("emitter", -1)) >= 0 else prev
        order[id(sh)] = (prev, int(sh.get("emitter", -1)) < 0, k)
    big = len(desc.emitters)
    shapes.sort(key=lambda rec: order[id(rec[1])] if rec[0] == "shape" else ((big, True, 0) if em_of(rec) < 0 else (em_of(rec), False, 0)))
    for gi, (kind, rec) in enumerate(shapes):
        if kind == "shape":  # a disk's toWorld as it is; a cylinder along z with its radius and length under the rotation that is left
            out.append('\t<shape type="%s">' % rec["type"])
            M4 = np.eye(4, dtype=np.float64); M4[:3, :] = np.asarray(rec["to_world"], np.float32).reshape(3, 4)
            out.append('\t\t<transform name="toWorld"><matrix value="%s"/></transform>' % " ".join(repr(float(x)) for x in M4.reshape(-1)))
            if rec["type"] == "cylinder":
                out.append('\t\t<point name="p1" x="0.0" y="0.0" z="%r"/>' % float(np.float32(rec["length"])))
                out.append('\t\t<float name="radius" value="%r"/>' % float(np.float32(rec["radius"])))
            if rec.get("flip_normals"):
                out.append('\t\t<boolean name="flipNormals" value="true"/>')
            out.append('\t\t<ref id="mat%d"/>' % int(rec.get("material", 0)))
            if int(rec.get("emitter", -1)) >= 0:
                out.append('\t\t<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % c(desc.emitters[int(rec["emitter"])]["radiance"]))
            out.append('\t</shape>')
            continue
        if kind == "sphere":
            out.append('\t<shape type="sphere">')
            R = np.asarray(rec.get("to_world", np.eye(3)), np.float32).reshape(3, 3)
            if np.array_equal(R, np.eye(3, dtype=np.float32)):
                out.append('\t\t<point name="center" x="%r" y="%r" z="%r"/>' % tuple(float(np.float32(v)) for v in rec["center"]))
            else:
                M4 = np.eye(4, dtype=np.float32); M4[:3, :3] = R; M4[:3, 3] = rec["center"]
                out.append('\t\t<transform name="toWorld"><matrix value="%s"/></transform>' % " ".join(repr(float(x)) for x in M4.reshape(-1)))
            out.append('\t\t<float name="radius" value="%r"/>' % float(np.float32(rec["radius"])))
            if rec.get("flip_normals"):
                out.append('\t\t<boolean name="flipNormals" value="true"/>')
            out.append('\t\t<ref id="mat%d"/>' % int(rec.get("material", 0)))
            if int(rec.get("emitter", -1)) >= 0:
                out.append('\t\t<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % c(desc.emitters[int(rec["emitter"])]["radiance"]))
            out.append('\t</shape>')
            continue
        mat, em = rec
        sel = np.nonzero((tm == mat) & (te == em))[0]
        fn = "meshes/%s_%03d.obj" % (name, gi)
        with open(os.path.join(directory, fn), "w") as f:
            used = np.unique(idx[sel])
            remap = {int(v): k + 1 for k, v in enumerate(used)}
            for v in used:
                f.write("v %r %r %r\n" % tuple(float(x) for x in pos[v]))
            if desc.normals is not None:
                for v in used:
                    f.write("vn %r %r %r\n" % tuple(float(x) for x in np.asarray(desc.normals)[v]))
            for t in sel:
                f.write("f " + " ".join(("%d//%d" % (remap[int(v)], remap[int(v)])) if desc.normals is not None else str(remap[int(v)]) for v in idx[t]) + "\n")
        out.append('\t<shape type="obj">')
        out.append('\t\t<string name="filename" value="%s"/>' % fn)
        if desc.normals is None:
            out.append('\t\t<boolean name="faceNormals" value="true"/>')
        out.append('\t\t<ref id="mat%d"/>' % mat)
        if em >= 0:
            out.append('\t\t<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % c(desc.emitters[em]["radiance"]))
        out.append('\t</shape>')
    for e in getattr(desc, "delta_emitters", None) or []:  # (the loader turns the values back into the same struct up to rounding)
        xyz = lambda v: 'x="%r" y="%r" z="%r"' % tuple(float(t) for t in v)  # noqa: E731
        if e["type"] == "point":
            out.append('\t<emitter type="point"><point name="position" %s/><rgb name="intensity" value="%s"/></emitter>' % (xyz(e["position"]), c(e["intensity"])))
        elif e["type"] == "directional":
            out.append('\t<emitter type="directional"><vector name="direction" %s/><rgb name="irradiance" value="%s"/></emitter>' % (xyz(e["direction"]), c(e["intensity"])))
        else:
            m = np.eye(4)
            m[:3, :3] = np.linalg.inv(np.asarray(e["to_local"], np.float64).reshape(3, 3))
            m[:3, 3] = e["position"]
            out.append('\t<emitter type="spot"><transform name="toWorld"><matrix value="%s"/></transform><float name="cutoffAngle" value="%r"/>'
                       '<float name="beamWidth" value="%r"/><rgb name="intensity" value="%s"/></emitter>'
                       % (" ".join(repr(float(x)) for x in m.reshape(-1)), math.degrees(e["cutoff_angle"]), math.degrees(e["beam_width"]), c(e["intensity"])))
    if getattr(desc, "environment", None) is not None:
        out.append('\t<emitter type="constant"><rgb name="radiance" value="%s"/></emitter>' % c(desc.environment))
    if getattr(desc, "envmap", None) is not None:
        from . import imageio
        imageio.write_pfm(os.path.join(directory, name + "_envmap.pfm"), desc.envmap["rgb"])
        M4 = np.eye(4, dtype=np.float32); M4[:3, :3] = np.asarray(desc.envmap.get("to_world", np.eye(3)), np.float32).reshape(3, 3)
        out.append('\t<emitter type="envmap"><string name="filename" value="%s_envmap.pfm"/><float name="scale" value="%r"/>'
                   '<transform name="toWorld"><matrix value="%s"/></transform></emitter>'
                   % (name, float(desc.envmap.get("scale", 1.0)), " ".join(repr(float(x)) for x in M4.reshape(-1))))
    out.append('</scene>')
    path = os.path.join(directory, name + ".xml")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return path
