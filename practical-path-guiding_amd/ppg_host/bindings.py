"""ctypes binding of include/ppg.h.

The product path is `Engine.hip()`: it loads practical-path-guiding_amd/lib/libppg_hip.so and raises
if the library is missing — there is no CPU fallback.  `Engine(lib, prefix="ppgo_")` lets tests/ and
bench.py's cpu_baseline drive the oracle through the identical call sequence.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)


def hip_library_path():
    # PPG_HIP_LIB selects an alternative build of the same library (kernel tuning A/B runs)
    return os.environ.get("PPG_HIP_LIB") or os.path.join(_PKG, "lib", "libppg_hip.so")


class PPGError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ppg error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    """ppg_config — property names and defaults of guided_path.cpp:1014-1085 / integrator.cpp:190-225."""
    _fields_ = [
        ("nee", C.c_char_p), ("sampleCombination", C.c_char_p), ("spatialFilter", C.c_char_p),
        ("directionalFilter", C.c_char_p), ("bsdfSamplingFractionLoss", C.c_char_p),
        ("sdTreeMaxMemory", C.c_int32), ("sTreeThreshold", C.c_int32), ("dTreeThreshold", C.c_float),
        ("bsdfSamplingFraction", C.c_float), ("sppPerPass", C.c_int32), ("budgetType", C.c_char_p),
        ("budget", C.c_float), ("dumpSDTree", C.c_int32), ("rrDepth", C.c_int32), ("maxDepth", C.c_int32),
        ("strictNormals", C.c_int32), ("hideEmitters", C.c_int32), ("seed", C.c_uint64), ("device", C.c_int32),
        ("dumpPrefix", C.c_char_p),
    ]

    DEFAULTS = dict(nee="never", sampleCombination="automatic", spatialFilter="nearest", directionalFilter="nearest",
                    bsdfSamplingFractionLoss="none", sdTreeMaxMemory=-1, sTreeThreshold=12000, dTreeThreshold=0.01,
                    bsdfSamplingFraction=0.5, sppPerPass=4, budgetType="seconds", budget=300.0, dumpSDTree=0,
                    rrDepth=5, maxDepth=-1, strictNormals=0, hideEmitters=0, seed=0, device=0, dumpPrefix=None)

    @classmethod
    def make(cls, **props):
        unknown = set(props) - set(cls.DEFAULTS)
        if unknown:
            raise KeyError("unknown integrator properties: %s" % sorted(unknown))
        vals = dict(cls.DEFAULTS)
        vals.update(props)
        cfg = cls()
        cfg._keep = []
        for k, v in vals.items():
            if isinstance(v, str):
                v = v.encode()
                cfg._keep.append(v)
            if isinstance(v, bool):
                v = int(v)
            setattr(cfg, k, v)
        return cfg


class Material(C.Structure):
    """ppg_material (include/ppg.h).  Scene descriptions carry materials as dicts: type, reflectance and — by type —
    specular, alpha, eta (3 values, or one number for plastic / dielectric), k, twosided, nonlinear, opacity (a mask adapter), distribution ("ggx" | "beckmann"), rtrans (roughplastic: row of SceneDesc.rtrans).
    The rest of the microfacet model travels beside it (Microfacet): alpha_v, distribution = "phong", sample_visible; so does a coating /
    roughcoating adapter around the BSDF (Coating): coating = dict(kind, eta, ...), and a blendbsdf / mixturebsdf of other materials (Blend):
    blend = dict(kind, children, ...).
    roughdiffuse: reflectance, alpha (0.2), fast_approx; difftrans: reflectance (its transmittance); phong: reflectance (diffuse), specular (0.2),
    exponent (30) — the HIP library only.  So are type = "null" (the pass-through BSDF: no other key applies) and normal_map = the index
    into SceneDesc.textures of a normalmap adapter's RGB normal map, which takes the place of `bump` (the two are exclusive)."""
    _fields_ = [("type", C.c_int32), ("reflectance", C.c_float * 3), ("specular", C.c_float * 3), ("alpha", C.c_float),
                ("eta", C.c_float * 3), ("k", C.c_float * 3), ("flags", C.c_int32), ("rtrans", C.c_int32),
                ("opacity", C.c_float * 3), ("texture", C.c_uint32)]

    BSDF = dict(diffuse=0, twosided_diffuse=1, mirror=2, conductor=3, roughconductor=4, plastic=5, dielectric=6, thindielectric=7, roughdielectric=8, roughplastic=9,
                roughdiffuse=10, difftrans=11, phong=12, null=13)
    LOBES = (10, 11, 12)  # the types only the HIP library knows
    NULL = 13             # ... and the pass-through BSDF, likewise
    NORMALMAP = 32            # PPG_MAT_NORMALMAP

    @classmethod
    def from_dict(cls, m):
        def three(v, default):
            v = default if v is None else v
            v = [v] * 3 if np.isscalar(v) else list(v)
            return [float(np.float32(x)) for x in v]
        o = cls()
        t = m.get("type", 0)
        o.type = cls.BSDF[t] if isinstance(t, str) else int(t)
        o.reflectance[:] = three(m.get("reflectance"), 0.5 if o.type in (0, 1, 5, 9, 10, 11, 12) else 1.0)
        o.specular[:] = three(m.get("specular"), 0.2 if o.type == 12 else 1.0)
        o.alpha = float(m.get("alpha", 0.2 if o.type == 10 else 0.1))
        if o.type == 12:  # phong: the record's alpha carries the exponent
            o.alpha = float(m.get("exponent", m.get("alpha", 30.0)))
        o.eta[:] = three(m.get("eta"), 0.0 if o.type in (2, 3, 4) else 1.5046)  # dielectric / plastic default: bk7 / polypropylene-ish
        o.k[:] = three(m.get("k"), 1.0)
        o.flags = ((1 if m.get("twosided") else 0) | (2 if m.get("nonlinear") else 0) | (4 if m.get("opacity") is not None else 0)
                   | (8 if m.get("distribution", "ggx") == "beckmann" else 0) | (16 if m.get("fast_approx") else 0))
        o.opacity[:] = three(m.get("opacity"), 0.0)
        o.rtrans = int(m.get("rtrans", 0))
        # texture: index into SceneDesc.textures of the bitmap on the diffuse reflectance; bump: of a bumpmap adapter's displacement texture
        # normal_map: of a normalmap adapter's normal map, in the same half of the word, with PPG_MAT_NORMALMAP
        tex, bump, nmap = m.get("texture"), m.get("bump"), m.get("normal_map")
        if bump is not None and nmap is not None:
            raise ValueError("a material states either `bump` or `normal_map`, not both (bump=%r, normal_map=%r)" % (bump, nmap))
        if nmap is not None:
            o.flags |= cls.NORMALMAP
            bump = nmap
        o.texture = (0 if tex is None else int(tex) + 1) | ((0 if bump is None else int(bump) + 1) << 16)
        return o


class MaterialTextures(C.Structure):
    """ppg_material_textures (include/ppg.h): per material, 1 + index into SceneDesc.textures of the bitmap on `specular`, `alpha`, `opacity`
    (0 = none).  Material dicts carry them as specular_texture / alpha_texture / opacity_texture = the index."""
    _fields_ = [("specular", C.c_uint32), ("alpha", C.c_uint32), ("opacity", C.c_uint32), ("_reserved", C.c_uint32)]

    KEYS = ("specular_texture", "alpha_texture", "opacity_texture")

    @classmethod
    def from_dict(cls, m):
        o = cls()
        o.specular, o.alpha, o.opacity = (0 if m.get(k) is None else int(m[k]) + 1 for k in cls.KEYS)
        return o


class Microfacet(C.Structure):
    """ppg_microfacet (include/ppg.h): per material, the part of Mitsuba's MicrofacetDistribution that ppg_material does not carry.  Material
    dicts state it as alpha_v (alphaV; `alpha` is then alphaU), alpha_v_texture (index into SceneDesc.textures), distribution = "phong" (or
    "as") and sample_visible = False.  A dict with any of these gets general = 1, also when alpha_v == alpha; every other an all-zero entry."""
    _fields_ = [("alpha_v", C.c_float), ("distribution", C.c_int32), ("sample_all", C.c_int32), ("alpha_v_texture", C.c_uint32),
                ("general", C.c_uint32), ("_reserved", C.c_uint32 * 3)]

    @staticmethod
    def is_general(m):
        return (m.get("alpha_v") is not None or m.get("alpha_v_texture") is not None or m.get("distribution") in ("phong", "as")
                or m.get("sample_visible", True) is False)

    @classmethod
    def from_dict(cls, m):
        o = cls()
        if not cls.is_general(m):
            return o
        o.general = 1
        o.alpha_v = float(m.get("alpha_v", m.get("alpha", 0.1)))
        o.distribution = 1 if m.get("distribution") in ("phong", "as") else 0
        o.sample_all = 0 if m.get("sample_visible", True) else 1
        o.alpha_v_texture = 0 if m.get("alpha_v_texture") is None else int(m["alpha_v_texture"]) + 1
        return o


class Coating(C.Structure):
    """ppg_coating (include/ppg.h): per material, Mitsuba's `coating` / `roughcoating` adapter around its BSDF (inside twosided / mask /
    bumpmap).  Material dicts state it as coating = dict(kind = "coating" | "roughcoating" (or 1 | 2; 0: none), eta (intIOR / extIOR,
    default bk7 / air), thickness (1), sigma_a (0), specular (1) and, for a roughcoating, alpha (0.1), distribution ("beckmann" | "ggx" |
    "phong"), sample_visible (True) and slice (or rtrans): the layer's row of SceneDesc.rtrans —
    rtrans.roughplastic_slice(distribution, alpha, eta, data_dir)).  A dict without the key gets an all-zero entry."""
    _fields_ = [("kind", C.c_int32), ("eta", C.c_float), ("thickness", C.c_float), ("sigma_a", C.c_float * 3), ("specular", C.c_float * 3),
                ("alpha", C.c_float), ("distribution", C.c_int32), ("sample_all", C.c_int32), ("rtrans", C.c_int32), ("_reserved", C.c_uint32 * 3)]

    KINDS = {"none": 0, "coating": 1, "roughcoating": 2}
    DISTRIBUTIONS = {"beckmann": 0, "ggx": 1, "phong": 2, "as": 2}
    BK7_OVER_AIR = 1.5046 / 1.000277  # ior.h: the plug-ins' default intIOR / extIOR

    @classmethod
    def from_dict(cls, m):
        """m: a material dict (its `coating` key) or the coating dict itself"""
        c = m if (m is not None and "kind" in m) else (m or {}).get("coating")
        o = cls()
        if c is None:
            return o
        def three(v, default):
            v = default if v is None else v
            v = [v] * 3 if np.isscalar(v) else list(v)
            return [float(np.float32(x)) for x in v]
        k = c.get("kind", 1)
        o.kind = cls.KINDS[k] if isinstance(k, str) else int(k)
        o.eta = float(np.float32(c.get("eta", cls.BK7_OVER_AIR)))
        o.thickness = float(c.get("thickness", 1.0))
        o.sigma_a[:] = three(c.get("sigma_a"), 0.0)
        o.specular[:] = three(c.get("specular"), 1.0)
        if o.kind == 2:
            o.alpha = float(c.get("alpha", 0.1))
            d = c.get("distribution", "beckmann")
            o.distribution = cls.DISTRIBUTIONS[d] if isinstance(d, str) else int(d)
            o.sample_all = 0 if c.get("sample_visible", True) else 1
            o.rtrans = int(c.get("rtrans", c.get("slice", 0)))  # (an index, not the slice's samples)
        return o

    def as_dict(self):
        """the material dict's `coating` value (None for kind 0)"""
        if self.kind == 0:
            return None
        d = dict(kind={1: "coating", 2: "roughcoating"}.get(self.kind, self.kind), eta=float(self.eta), thickness=float(self.thickness),
                 sigma_a=[float(v) for v in self.sigma_a], specular=[float(v) for v in self.specular])
        if self.kind == 2:
            d.update(alpha=float(self.alpha), distribution={0: "beckmann", 1: "ggx", 2: "phong"}.get(self.distribution, self.distribution),
                     sample_visible=not self.sample_all, slice=int(self.rtrans))
        return d


class Blend(C.Structure):
    """ppg_blend (include/ppg.h): per material, Mitsuba's `blendbsdf` / `mixturebsdf` over other entries of the material list.  Material
    dicts state it as blend = dict(kind = "blendbsdf" | "mixturebsdf" (or 1 | 2; 0: none), children = [material dicts, or indices into the
    material list], and — blendbsdf — weight (0.5), weight_texture (index into SceneDesc.textures, or None) or — mixturebsdf — weights (one
    per child) and ensure_energy_conservation (True)).  The dict that carries it is the blended material's own record: type 0, with
    twosided / opacity / opacity_texture / bump around the blend.  expand_blends appends children given as dicts to the material list; a
    dict without the key gets an all-zero entry."""
    _fields_ = [("kind", C.c_int32), ("n", C.c_uint32), ("child", C.c_uint32 * 4), ("weight", C.c_float * 4), ("weight_texture", C.c_uint32),
                ("ensure_energy_conservation", C.c_int32), ("_reserved", C.c_uint32 * 4)]

    KINDS = {"none": 0, "blendbsdf": 1, "mixturebsdf": 2}
    MAX = 4  # PPG_BLEND_MAX

    @classmethod
    def from_dict(cls, m):
        """m: a material dict (its `blend` key) or the blend dict itself, its children given as indices"""
        b = m if (m is not None and "children" in m) else (m or {}).get("blend")
        o = cls()
        if b is None:
            return o
        k = b.get("kind", 1)
        o.kind = cls.KINDS[k] if isinstance(k, str) else int(k)
        if o.kind == 0:
            return o
        kids = list(b["children"])
        if any(isinstance(c, dict) for c in kids):
            raise ValueError("blend: children given as dicts belong to a material list (bindings.expand_blends)")
        if len(kids) > cls.MAX:
            raise ValueError("blend: more than %d children are not supported (found %d)" % (cls.MAX, len(kids)))
        o.n = len(kids)
        for i, c in enumerate(kids):
            o.child[i] = int(c)
        if o.kind == 1:
            o.weight[0] = float(b.get("weight", 0.5))
            t = b.get("weight_texture")
            o.weight_texture = 0 if t is None else int(t) + 1
        else:
            w = [float(v) for v in b.get("weights", [])]
            if len(w) != len(kids):
                raise ValueError("blend: BSDF count mismatch: %d bsdfs, but specified %d weights" % (len(kids), len(w)))
            for i, v in enumerate(w):
                o.weight[i] = v
            o.ensure_energy_conservation = 1 if b.get("ensure_energy_conservation", True) else 0
        return o

    def as_dict(self):
        """the material dict's `blend` value (None for kind 0)"""
        if self.kind == 0:
            return None
        d = dict(kind={1: "blendbsdf", 2: "mixturebsdf"}.get(self.kind, self.kind), children=[int(self.child[i]) for i in range(min(self.n, self.MAX))])
        if self.kind == 1:
            d.update(weight=float(self.weight[0]), weight_texture=int(self.weight_texture) - 1 if self.weight_texture else None)
        else:
            d.update(weights=[float(self.weight[i]) for i in range(min(self.n, self.MAX))], ensure_energy_conservation=bool(self.ensure_energy_conservation))
        return d


class Medium(C.Structure):
    """ppg_medium (include/ppg.h): a homogeneous medium (medium/homogeneous.cpp) with its phase function.  Scene descriptions carry media
    as dicts (SceneDesc.media): sigma_a + sigma_s, or sigma_t + albedo (sigma_s = sigma_t * albedo, sigma_a = sigma_t - sigma_s, as
    medium.cpp derives them), each a number or an RGB triple; scale (1) multiplies both; strategy ("balance" | "single" | "manual"),
    channel (single; None: the smallest sigma_t), sampling_density (manual), sampling_weight (None: derive it), phase ("isotropic" | "hg"), g.
    A heterogeneous medium (medium/heterogeneous.cpp, Woodcock tracking) reads dict(type="heterogeneous", density=V, albedo=V, scale=1.0,
    phase=.., g=..) with V a volume dict (Volume): its record here keeps phase and g and zero coefficients, and flatten_media_volumes
    makes the entry of ppg_set_media_volumes' list that names it."""
    _fields_ = [("sigma_a", C.c_float * 3), ("sigma_s", C.c_float * 3), ("strategy", C.c_int32), ("channel", C.c_int32),
                ("sampling_density", C.c_float), ("sampling_weight", C.c_float), ("phase", C.c_int32), ("g", C.c_float), ("_reserved", C.c_uint32 * 4)]
    STRATEGIES = ("balance", "single", "manual")
    PHASES = ("isotropic", "hg")

    @classmethod
    def from_dict(cls, d):
        def rgb(v):
            a = np.asarray(v, np.float32).reshape(-1)
            return np.repeat(a, 3) if a.size == 1 else a
        m = cls()
        scale = np.float32(d.get("scale", 1.0))
        if d.get("type") == "heterogeneous":  # (density, albedo and scale travel in ppg_set_media_volumes' list: flatten_media_volumes)
            for k in ("sigma_a", "sigma_s", "sigma_t", "strategy", "channel", "sampling_density", "sampling_weight"):
                if k in d:
                    raise ValueError("heterogeneous medium: %r belongs to homogeneous media; give `density` and `albedo` volumes" % k)
            if "density" not in d or "albedo" not in d:
                raise ValueError("heterogeneous medium: state `density` and `albedo` volumes")
            sa = ss = np.zeros(3, np.float32)
        elif "sigma_t" in d or "albedo" in d:
            if "sigma_a" in d or "sigma_s" in d or "sigma_t" not in d or "albedo" not in d:
                raise ValueError("medium: state sigma_a and sigma_s, or sigma_t and albedo")
            st = rgb(d["sigma_t"]) * scale   # medium.cpp: the scale first, then sigmaS = sigmaT * albedo, sigmaA = sigmaT - sigmaS
            ss = st * rgb(d["albedo"])
            sa = st - ss
        else:
            if "sigma_a" not in d or "sigma_s" not in d:
                raise ValueError("medium: state sigma_a and sigma_s, or sigma_t and albedo")
            sa, ss = rgb(d["sigma_a"]) * scale, rgb(d["sigma_s"]) * scale
        m.sigma_a[:] = [float(v) for v in sa]
        m.sigma_s[:] = [float(v) for v in ss]
        strategy = d.get("strategy", "balance")
        m.strategy = cls.STRATEGIES.index(strategy) if isinstance(strategy, str) else int(strategy)
        channel = d.get("channel")
        m.channel = -1 if channel is None else int(channel)
        m.sampling_density = float(d.get("sampling_density", 0.0))
        weight = d.get("sampling_weight")
        m.sampling_weight = -1.0 if weight is None else float(weight)
        phase = d.get("phase", "isotropic")
        m.phase = cls.PHASES.index(phase) if isinstance(phase, str) else int(phase)
        m.g = float(d.get("g", 0.0))
        return m


class Media(C.Structure):
    """ppg_media (include/ppg.h)"""
    _fields_ = [("n_media", C.c_uint32), ("camera_medium", C.c_uint32), ("media", C.POINTER(Medium)),
                ("n_tri_media", C.c_uint32), ("n_sphere_media", C.c_uint32), ("n_shape_media", C.c_uint32), ("_reserved", C.c_uint32),
                ("tri_media", C.POINTER(C.c_uint32)), ("sphere_media", C.POINTER(C.c_uint32)), ("shape_media", C.POINTER(C.c_uint32))]


class Volume(C.Structure):
    """ppg_volume (include/ppg.h): a constant or a grid volume.  Media dicts carry volumes as dicts: dict(value=0.5 | (r, g, b)), or
    dict(data=ndarray[z, y, x] | [z, y, x, 3], min=(x, y, z), max=(x, y, z), to_world=4x4 (None: the identity))."""
    _fields_ = [("kind", C.c_int32), ("channels", C.c_int32), ("value", C.c_float * 3), ("res", C.c_int32 * 3), ("aabb_min", C.c_float * 3),
                ("aabb_max", C.c_float * 3), ("to_world", C.c_float * 16), ("_reserved", C.c_uint32 * 2), ("data", C.POINTER(C.c_float))]
    CONST, GRID = 0, 1

    @classmethod
    def from_dict(cls, d, channels, keep):
        """`channels`: what the volume is asked for (1: density, 3: albedo) — a const value given as one number serves both; `keep`
        receives the arrays the record points into."""
        v = cls()
        if "value" in d:
            a = np.asarray(d["value"], np.float32).reshape(-1)
            if a.size not in (1, 3) or (a.size == 3 and channels == 1):
                raise ValueError("volume: a const %s takes %s" % ("density" if channels == 1 else "albedo", "one number" if channels == 1 else "a number or an RGB triple"))
            a = np.repeat(a, 3) if (a.size == 1 and channels == 3) else a
            v.kind, v.channels = cls.CONST, int(a.size)
            v.value[:a.size] = [float(x) for x in a]
            return v
        data = np.ascontiguousarray(d["data"], np.float32)
        if data.ndim not in (3, 4) or (data.ndim == 4 and data.shape[3] not in (1, 3)):
            raise ValueError("volume: data must be [z, y, x] or [z, y, x, 3]")
        keep.append(data)
        v.kind, v.channels = cls.GRID, (1 if data.ndim == 3 else int(data.shape[3]))
        v.res[:] = [int(data.shape[2]), int(data.shape[1]), int(data.shape[0])]
        v.aabb_min[:] = [float(x) for x in np.asarray(d["min"], np.float32).reshape(3)]
        v.aabb_max[:] = [float(x) for x in np.asarray(d["max"], np.float32).reshape(3)]
        tw = d.get("to_world")
        v.to_world[:] = [float(x) for x in (np.eye(4, dtype=np.float32) if tw is None else np.asarray(tw, np.float32).reshape(4, 4)).reshape(-1)]
        v.data = data.ctypes.data_as(C.POINTER(C.c_float))
        return v


class MediumVolumes(C.Structure):
    """ppg_medium_volumes (include/ppg.h)"""
    _fields_ = [("medium", C.c_uint32), ("density", C.c_uint32), ("albedo", C.c_uint32), ("scale", C.c_float), ("_reserved", C.c_uint32 * 4)]


class MediaVolumes(C.Structure):
    """ppg_media_volumes (include/ppg.h)"""
    _fields_ = [("n_volumes", C.c_uint32), ("n_entries", C.c_uint32), ("volumes", C.POINTER(Volume)), ("entries", C.POINTER(MediumVolumes)),
                ("_reserved", C.c_uint32 * 4)]


def flatten_media_volumes(media):
    """The side list of ppg_set_media_volumes for a list of medium dicts: (volumes, entries) — every heterogeneous medium's `density` and
    `albedo` dicts as Volume records (a dict that two media share is one volume) and one MediumVolumes entry per such medium —, and the
    arrays they point into."""
    volumes, entries, keep, seen = [], [], [], {}

    def volume(d, channels):
        key = (id(d), channels)
        if key not in seen:
            seen[key] = len(volumes)
            volumes.append(Volume.from_dict(d, channels, keep))
        return seen[key]
    for i, m in enumerate(media or []):
        if isinstance(m, dict) and m.get("type") == "heterogeneous":
            e = MediumVolumes()
            e.medium, e.density, e.albedo, e.scale = i, volume(m["density"], 1), volume(m["albedo"], 3), float(m.get("scale", 1.0))
            entries.append(e)
    return volumes, entries, keep


def media_word(interior=None, exterior=None):
    """The binding word of a primitive (ppg_media): low 16 bits = 1 + the interior medium's index, high 16 bits = 1 + the exterior one's."""
    return (0 if interior is None else 1 + int(interior)) | ((0 if exterior is None else 1 + int(exterior)) << 16)


def has_media(desc):
    """Whether `desc` carries participating media (what the CPU oracle, the .ppgs container and the C++ loader do not implement)."""
    return bool(getattr(desc, "media", None))


class DebugMediumItem(C.Structure):
    _fields_ = [("medium", C.c_int32), ("length", C.c_float), ("wi", C.c_float * 3), ("u", C.c_float * 4)]


class DebugMediumOut(C.Structure):
    _fields_ = [("success", C.c_int32), ("t", C.c_float), ("pdf_success", C.c_float), ("pdf_failure", C.c_float), ("transmittance", C.c_float * 3),
                ("eval_transmittance", C.c_float * 3), ("wo", C.c_float * 3), ("phase_eval", C.c_float), ("phase_pdf", C.c_float)]


class DebugVolumeItem(C.Structure):
    _fields_ = [("volume", C.c_int32), ("p", C.c_float * 3)]


class DebugVolumeOut(C.Structure):
    _fields_ = [("value", C.c_float * 3)]


class DebugHetmediumItem(C.Structure):
    _fields_ = [("medium", C.c_int32), ("o", C.c_float * 3), ("d", C.c_float * 3), ("maxt", C.c_float), ("key", C.c_uint32), ("dim", C.c_uint32)]


class DebugHetmediumOut(C.Structure):
    _fields_ = [("success", C.c_int32), ("t", C.c_float), ("sigma_s", C.c_float * 3), ("transmittance", C.c_float), ("draws", C.c_uint32),
                ("eval_transmittance", C.c_float), ("eval_draws", C.c_uint32)]


DEBUG_VOLUME_ITEM_DTYPE = np.dtype([("volume", "<i4"), ("p", "<f4", 3)])
DEBUG_VOLUME_OUT_DTYPE = np.dtype([("value", "<f4", 3)])
DEBUG_HETMEDIUM_ITEM_DTYPE = np.dtype([("medium", "<i4"), ("o", "<f4", 3), ("d", "<f4", 3), ("maxt", "<f4"), ("key", "<u4"), ("dim", "<u4")])
DEBUG_HETMEDIUM_OUT_DTYPE = np.dtype([("success", "<i4"), ("t", "<f4"), ("sigma_s", "<f4", 3), ("transmittance", "<f4"), ("draws", "<u4"),
                                      ("eval_transmittance", "<f4"), ("eval_draws", "<u4")])
DEBUG_MEDIUM_ITEM_DTYPE = np.dtype([("medium", "<i4"), ("length", "<f4"), ("wi", "<f4", 3), ("u", "<f4", 4)])
DEBUG_MEDIUM_OUT_DTYPE = np.dtype([("success", "<i4"), ("t", "<f4"), ("pdf_success", "<f4"), ("pdf_failure", "<f4"), ("transmittance", "<f4", 3),
                                   ("eval_transmittance", "<f4", 3), ("wo", "<f4", 3), ("phase_eval", "<f4"), ("phase_pdf", "<f4")])


def has_blends(desc):
    """Whether a material of `desc` carries a `blend` entry (what the CPU oracle does not implement)."""
    return any(m.get("blend") is not None for m in desc.materials)


def expand_blends(materials):
    """The material list with the children that blended materials state as dicts appended to it, in order, and named by their indices:
    what the C-ABI and the flat scene file hold.  A list without such children comes back as it is."""
    if not any(isinstance(c, dict) for m in materials if m.get("blend") is not None for c in m["blend"].get("children", [])):
        return materials
    out = list(materials)
    for i, m in enumerate(materials):
        b = m.get("blend")
        if b is None:
            continue
        kids = []
        for c in b.get("children", []):
            if isinstance(c, dict):
                out.append(c)
                kids.append(len(out) - 1)
            else:
                kids.append(int(c))
        out[i] = dict(m, blend=dict(b, children=kids))
    return out


def has_coatings(desc):
    """Whether a material of `desc` carries a `coating` entry (what the CPU oracle does not implement)."""
    return any(m.get("coating") is not None for m in desc.materials)


def has_general_microfacet(desc):
    """Whether a material of `desc` needs an entry of ppg_set_microfacet (what the CPU oracle does not implement)."""
    return any(Microfacet.is_general(m) for m in desc.materials)


def has_parameter_textures(desc):
    """Whether a material of `desc` carries a bitmap on specular / alpha / opacity (what the CPU oracle does not implement)."""
    return any(m.get(k) is not None for m in desc.materials for k in MaterialTextures.KEYS)


class Sphere(C.Structure):
    """ppg_sphere (include/ppg.h).  Scene descriptions carry spheres as dicts: center, radius, material, emitter (-1), flip_normals,
    to_world (9 floats, row-major rotation; identity by default)."""
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("to_world", C.c_float * 9), ("material", C.c_uint32),
                ("emitter", C.c_int32), ("flip_normals", C.c_int32)]

    @classmethod
    def from_dict(cls, d):
        o = cls()
        o.center[:] = [float(np.float32(v)) for v in d["center"]]
        o.radius = float(np.float32(d["radius"]))
        o.to_world[:] = [float(np.float32(v)) for v in np.asarray(d.get("to_world", np.eye(3)), np.float32).reshape(-1)]
        o.material, o.emitter, o.flip_normals = int(d.get("material", 0)), int(d.get("emitter", -1)), 1 if d.get("flip_normals") else 0
        return o


class Shape(C.Structure):
    """ppg_shape (include/ppg.h) — an analytic disk or cylinder.  Scene descriptions carry them as dicts (SceneDesc.shapes): type ("disk" |
    "cylinder"), to_world (12 floats, row-major 3x4: the disk's toWorld; the cylinder's object-to-world with its scale removed), radius and
    length (cylinder), material, emitter (-1), flip_normals."""
    TYPES = ("disk", "cylinder")
    _fields_ = [("type", C.c_int32), ("to_world", C.c_float * 12), ("radius", C.c_float), ("length", C.c_float), ("material", C.c_uint32),
                ("emitter", C.c_int32), ("flip_normals", C.c_int32), ("_reserved", C.c_uint32 * 2)]

    @classmethod
    def from_dict(cls, d):
        unknown = set(d) - {"type", "to_world", "radius", "length", "material", "emitter", "flip_normals"}
        if unknown:
            raise ValueError("shape: unknown parameters %s" % sorted(unknown))
        o = cls()
        t = d.get("type")
        o.type = cls.TYPES.index(t) if t in cls.TYPES else int(t)  # (an unknown number is ppg_set_scene's to refuse)
        o.to_world[:] = [float(np.float32(v)) for v in np.asarray(d.get("to_world", np.eye(4)[:3]), np.float32).reshape(-1)]
        o.radius, o.length = float(np.float32(d.get("radius", 0.0))), float(np.float32(d.get("length", 0.0)))
        o.material, o.emitter, o.flip_normals = int(d.get("material", 0)), int(d.get("emitter", -1)), 1 if d.get("flip_normals") else 0
        return o

    def as_dict(self):
        d = dict(type=self.TYPES[self.type], to_world=[float(v) for v in self.to_world], material=int(self.material), emitter=int(self.emitter),
                 flip_normals=bool(self.flip_normals))
        if self.type == 1:
            d.update(radius=float(self.radius), length=float(self.length))
        return d


class DebugHit(C.Structure):
    """ppg_debug_hit (include/ppg_testhooks.h)"""
    _fields_ = [("prim", C.c_int32), ("t", C.c_float), ("p", C.c_float * 3), ("geo_n", C.c_float * 3), ("n", C.c_float * 3), ("s", C.c_float * 3),
                ("wi", C.c_float * 3), ("material", C.c_int32), ("emitter", C.c_int32), ("_pad", C.c_int32)]


class DebugFrame(C.Structure):
    """ppg_debug_frame (include/ppg_testhooks.h)"""
    _fields_ = [("prim", C.c_int32), ("material", C.c_int32), ("uv", C.c_float * 2), ("n", C.c_float * 3), ("s", C.c_float * 3),
                ("ps", C.c_float * 3), ("pt", C.c_float * 3), ("pn", C.c_float * 3), ("adapted", C.c_int32)]


class DebugBsdfItem(C.Structure):
    """ppg_debug_bsdf_item (include/ppg_testhooks.h)"""
    _fields_ = [("material", C.c_int32), ("wi", C.c_float * 3), ("wo", C.c_float * 3), ("sample", C.c_float * 2), ("key", C.c_uint32), ("uv", C.c_float * 2)]


class DebugBsdfOut(C.Structure):
    """ppg_debug_bsdf_out (include/ppg_testhooks.h)"""
    _fields_ = [("eval", C.c_float * 3), ("pdf", C.c_float), ("wo", C.c_float * 3), ("sampled_pdf", C.c_float), ("weight", C.c_float * 3),
                ("eta", C.c_float), ("delta", C.c_int32), ("is_null", C.c_int32), ("_pad", C.c_int32 * 2)]


class DebugDirect(C.Structure):
    """ppg_debug_direct (include/ppg_testhooks.h)"""
    _fields_ = [("emitter", C.c_int32), ("d", C.c_float * 3), ("dist", C.c_float), ("n", C.c_float * 3), ("pdf", C.c_float), ("em_pdf", C.c_float),
                ("value", C.c_float * 3), ("_pad", C.c_float * 3)]


class DebugDirectEx(C.Structure):
    """ppg_debug_direct_ex (include/ppg_testhooks.h)"""
    _fields_ = [("emitter", C.c_int32), ("d", C.c_float * 3), ("dist", C.c_float), ("n", C.c_float * 3), ("pdf", C.c_float), ("em_pdf", C.c_float),
                ("value", C.c_float * 3), ("sd", C.c_float * 3), ("sdist", C.c_float), ("is_env", C.c_int32), ("is_delta", C.c_int32), ("_pad", C.c_int32)]


class DebugPdf(C.Structure):
    """ppg_debug_pdf (include/ppg_testhooks.h)"""
    _fields_ = [("prim", C.c_int32), ("emitter", C.c_int32), ("value", C.c_float * 3), ("pdf_direct", C.c_float), ("emitter_pdf", C.c_float), ("_pad", C.c_int32)]


DEBUG_HIT_DTYPE = np.dtype([("prim", "<i4"), ("t", "<f4"), ("p", "<f4", 3), ("geo_n", "<f4", 3), ("n", "<f4", 3), ("s", "<f4", 3), ("wi", "<f4", 3),
                            ("material", "<i4"), ("emitter", "<i4"), ("_pad", "<i4")])
DEBUG_FRAME_DTYPE = np.dtype([("prim", "<i4"), ("material", "<i4"), ("uv", "<f4", 2), ("n", "<f4", 3), ("s", "<f4", 3), ("ps", "<f4", 3), ("pt", "<f4", 3),
                              ("pn", "<f4", 3), ("adapted", "<i4")])
DEBUG_BSDF_ITEM_DTYPE = np.dtype([("material", "<i4"), ("wi", "<f4", 3), ("wo", "<f4", 3), ("sample", "<f4", 2), ("key", "<u4"), ("uv", "<f4", 2)])
DEBUG_BSDF_OUT_DTYPE = np.dtype([("eval", "<f4", 3), ("pdf", "<f4"), ("wo", "<f4", 3), ("sampled_pdf", "<f4"), ("weight", "<f4", 3), ("eta", "<f4"),
                                 ("delta", "<i4"), ("is_null", "<i4"), ("_pad", "<i4", 2)])
DEBUG_DIRECT_DTYPE = np.dtype([("emitter", "<i4"), ("d", "<f4", 3), ("dist", "<f4"), ("n", "<f4", 3), ("pdf", "<f4"), ("em_pdf", "<f4"),
                               ("value", "<f4", 3), ("_pad", "<f4", 3)])
DEBUG_DIRECT_EX_DTYPE = np.dtype([("emitter", "<i4"), ("d", "<f4", 3), ("dist", "<f4"), ("n", "<f4", 3), ("pdf", "<f4"), ("em_pdf", "<f4"),
                                  ("value", "<f4", 3), ("sd", "<f4", 3), ("sdist", "<f4"), ("is_env", "<i4"), ("is_delta", "<i4"), ("_pad", "<i4")])
DEBUG_PDF_DTYPE = np.dtype([("prim", "<i4"), ("emitter", "<i4"), ("value", "<f4", 3), ("pdf_direct", "<f4"), ("emitter_pdf", "<f4"), ("_pad", "<i4")])


MAX_FIELDS = 8  # PPG_MAX_FIELDS
# Mitsuba's names of the field integrator's fields (field.cpp:72-91) -> PPG_FIELD_*; `shapeIndex` is not offered (include/ppg.h)
FIELD_NAMES = dict(position=0, relPosition=1, distance=2, geoNormal=3, shNormal=4, uv=5, albedo=6, primIndex=7)


class Fields(C.Structure):
    """ppg_fields (include/ppg.h)"""
    _fields_ = [("n_fields", C.c_uint32), ("field", C.c_int32 * MAX_FIELDS), ("undefined", (C.c_float * 3) * MAX_FIELDS), ("spp", C.c_uint32),
                ("first_sample", C.c_uint32)]


def field_code(name):
    """PPG_FIELD_* of one of Mitsuba's field names; ValueError (listing the known ones) for any other"""
    if name not in FIELD_NAMES:
        raise ValueError("unknown field %r: the known fields are %s" % (name, ", ".join(FIELD_NAMES)))
    return FIELD_NAMES[name]


class DebugCommitIn(C.Structure):  # ppg_debug_commit_in
    _fields_ = [("route", C.c_int32), ("n_paths", C.c_uint32), ("n_vertices", C.c_uint64),
                ("nv", C.POINTER(C.c_uint32)), ("key", C.POINTER(C.c_uint32)), ("dim", C.POINTER(C.c_uint32)), ("late", C.POINTER(C.c_uint8)),
                ("p", C.POINTER(C.c_float)), ("d", C.POINTER(C.c_float)), ("radiance", C.POINTER(C.c_float)), ("throughput", C.POINTER(C.c_float)),
                ("bsdf_val", C.POINTER(C.c_float)), ("wo_pdf", C.POINTER(C.c_float)), ("bsdf_pdf", C.POINTER(C.c_float)),
                ("dtree_pdf", C.POINTER(C.c_float)), ("is_delta", C.POINTER(C.c_uint8))]


class DebugCommitOut(C.Structure):  # ppg_debug_commit_out
    _fields_ = [("committed", C.c_uint64), ("n_keys", C.c_uint64), ("keys_cap", C.c_uint64), ("keys", C.POINTER(C.c_uint64)),
                ("n_records", C.c_uint64), ("records_cap", C.c_uint64), ("records", C.c_void_p), ("adam_state", C.POINTER(C.c_uint32))]


# ppg_adam_record (include/ppg.h)
ADAM_RECORD_DTYPE = np.dtype([("key", np.uint64), ("product", np.float32), ("wo_pdf", np.float32), ("bsdf_pdf", np.float32),
                              ("dtree_pdf", np.float32), ("weight", np.float32), ("pad", np.float32)])


class EnvMap(C.Structure):
    """ppg_envmap (include/ppg.h).  Scene descriptions carry it as a dict: rgb (float32 [height, width, 3]), scale, to_world (9 floats)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_float)), ("scale", C.c_float), ("to_world", C.c_float * 9)]

    @classmethod
    def from_dict(cls, d):
        o = cls()
        rgb = np.ascontiguousarray(d["rgb"], np.float32)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        o.height, o.width = rgb.shape[0], rgb.shape[1]
        o.rgb = rgb.ctypes.data_as(C.POINTER(C.c_float))
        o.scale = float(np.float32(d.get("scale", 1.0)))
        o.to_world[:] = [float(np.float32(v)) for v in np.asarray(d.get("to_world", np.eye(3)), np.float32).reshape(-1)]
        o._keep = rgb
        return o


class Texture(C.Structure):
    """ppg_texture (include/ppg.h).  Scene descriptions carry textures as dicts: rgb (float32 [height, width, 3], linear), uv_scale, uv_offset,
    wrap_u / wrap_v ("repeat" | "mirror" | "clamp" | "zero" | "one"), nearest."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_float)), ("uv_scale", C.c_float * 2), ("uv_offset", C.c_float * 2),
                ("wrap_u", C.c_int32), ("wrap_v", C.c_int32), ("nearest", C.c_int32)]
    WRAP = dict(repeat=0, mirror=1, clamp=2, zero=3, one=4)

    @classmethod
    def from_dict(cls, d):
        o = cls()
        rgb = np.ascontiguousarray(d["rgb"], np.float32)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        o.height, o.width = rgb.shape[0], rgb.shape[1]
        o.rgb = rgb.ctypes.data_as(C.POINTER(C.c_float))
        o.uv_scale[:] = [float(np.float32(v)) for v in d.get("uv_scale", (1.0, 1.0))]
        o.uv_offset[:] = [float(np.float32(v)) for v in d.get("uv_offset", (0.0, 0.0))]
        wu, wv = d.get("wrap_u", "repeat"), d.get("wrap_v", "repeat")
        o.wrap_u = cls.WRAP[wu] if isinstance(wu, str) else int(wu)
        o.wrap_v = cls.WRAP[wv] if isinstance(wv, str) else int(wv)
        o.nearest = 1 if d.get("nearest") else 0
        o._keep = rgb
        return o


class RFilter(C.Structure):
    """ppg_rfilter — the film's reconstruction filter (mitsuba/src/rfilters/).  As a dict (SceneDesc.rfilter): {"type": name} plus the
    type's own parameters — box: radius, gaussian: stddev, mitchell: B, C, lanczos: lobes; None = the default box (radius 0.5)."""
    _fields_ = [("type", C.c_int32), ("radius", C.c_float), ("stddev", C.c_float), ("B", C.c_float), ("C", C.c_float), ("lobes", C.c_int32)]
    TYPES = ("box", "tent", "gaussian", "mitchell", "catmullrom", "lanczos")
    PARAMS = dict(box=("radius",), tent=(), gaussian=("stddev",), mitchell=("B", "C"), catmullrom=(), lanczos=("lobes",))
    DEFAULTS = dict(radius=0.5, stddev=0.5, B=1.0 / 3.0, C=1.0 / 3.0, lobes=3)

    @classmethod
    def from_dict(cls, d):
        d = d or {"type": "box"}
        t = d["type"]
        if t not in cls.TYPES:
            raise ValueError("unknown reconstruction filter %r" % (t,))
        unknown = set(d) - {"type"} - set(cls.PARAMS[t])
        if unknown:
            raise ValueError("%s filter: unknown parameters %s" % (t, sorted(unknown)))
        v = dict(cls.DEFAULTS, **{k: d[k] for k in cls.PARAMS[t] if k in d})
        return cls(cls.TYPES.index(t), v["radius"], v["stddev"], v["B"], v["C"], int(v["lobes"]))

    def as_dict(self):
        """None for the default box, else {"type", the type's parameters}"""
        t = self.TYPES[self.type]
        if t == "box" and self.radius == np.float32(0.5):
            return None
        d = {"type": t}
        for k in self.PARAMS[t]:
            d[k] = int(self.lobes) if k == "lobes" else float(getattr(self, k))
        return d


def rfilter_table(desc):
    """ppg_debug_rfilter_table (host only): (table float32[32], radius, border) of a filter dict (None = default box)."""
    lib = C.CDLL(hip_library_path())
    f = RFilter.from_dict(desc)
    table, r, b = np.zeros(32, np.float32), C.c_float(), C.c_int32()
    rc = lib.ppg_debug_rfilter_table(C.byref(f), _p(table, C.c_float), C.byref(r), C.byref(b))
    if rc != 0:
        raise PPGError(rc, "invalid reconstruction filter %r" % (desc,))
    return table, float(r.value), int(b.value)


def footprint_halo_floats(width, height, tile_size, world, border, lib=None):
    """ppg_footprint_halo_floats (host only): floats of the halo buffer a sharded filtered film exchanges — 7 per border slot, 0 for
    world <= 1 or border < 1 (include/ppg.h "Footprint hook")."""
    f = (lib or C.CDLL(hip_library_path())).ppg_footprint_halo_floats
    f.restype, f.argtypes = C.c_uint64, [C.c_int32] * 5
    return int(f(int(width), int(height), int(tile_size), int(world), int(border)))


class Lens(C.Structure):
    """ppg_lens — a thin-lens camera (mitsuba/src/sensors/thinlens.cpp).  As a dict (SceneDesc.lens): {"aperture_radius", "focus_distance"}
    in world units; None = pinhole."""
    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float)]

    @classmethod
    def from_dict(cls, d):
        unknown = set(d) - {"aperture_radius", "focus_distance"}
        if unknown:
            raise ValueError("thin lens: unknown parameters %s" % sorted(unknown))
        return cls(float(d["aperture_radius"]), float(d["focus_distance"]))

    def as_dict(self):
        return dict(aperture_radius=float(self.aperture_radius), focus_distance=float(self.focus_distance))


class DeltaEmitter(C.Structure):
    """ppg_delta_emitter — a point, spot or directional emitter (mitsuba/src/emitters/point.cpp, spot.cpp, directional.cpp).  As a dict
    (SceneDesc.delta_emitters): {"type": "point" | "spot" | "directional", "intensity": rgb (directional: the irradiance), and per type
    "position" (point, spot), "to_local": the 3x3 of toWorld's inverse, row-major, "cutoff_angle", "beam_width" in radians (spot),
    "direction" (directional)}."""
    TYPES = ("point", "spot", "directional")
    _fields_ = [("type", C.c_int32), ("intensity", C.c_float * 3), ("position", C.c_float * 3), ("to_local", C.c_float * 9),
                ("direction", C.c_float * 3), ("cutoff_angle", C.c_float), ("beam_width", C.c_float)]

    @classmethod
    def from_dict(cls, d):
        unknown = set(d) - {"type", "intensity", "position", "to_local", "direction", "cutoff_angle", "beam_width"}
        if unknown:
            raise ValueError("delta emitter: unknown parameters %s" % sorted(unknown))
        if d.get("type") not in cls.TYPES:
            raise ValueError("delta emitter: unknown type %r (point, spot, directional)" % (d.get("type"),))
        e = cls()
        e.type = cls.TYPES.index(d["type"])
        e.intensity[:] = [float(v) for v in d["intensity"]]
        e.position[:] = [float(v) for v in d.get("position", (0, 0, 0))]
        e.to_local[:] = [float(v) for v in np.asarray(d.get("to_local", np.eye(3)), np.float32).reshape(-1)]
        e.direction[:] = [float(v) for v in d.get("direction", (0, 0, 0))]
        e.cutoff_angle, e.beam_width = float(d.get("cutoff_angle", 0.0)), float(d.get("beam_width", 0.0))
        return e

    def as_dict(self):
        t = self.TYPES[self.type]
        d = dict(type=t, intensity=tuple(float(v) for v in self.intensity))
        if t != "directional":
            d["position"] = tuple(float(v) for v in self.position)
        if t == "spot":
            d.update(to_local=[float(v) for v in self.to_local], cutoff_angle=float(self.cutoff_angle), beam_width=float(self.beam_width))
        if t == "directional":
            d["direction"] = tuple(float(v) for v in self.direction)
        return d


class Emitter(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("_pad", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("sample_to_camera", C.c_float * 16), ("camera_to_world", C.c_float * 16),
                ("near_clip", C.c_float), ("far_clip", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


class Scene(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("n_triangles", C.c_uint32), ("indices", C.POINTER(C.c_uint32)), ("tri_material", C.POINTER(C.c_uint32)),
                ("tri_emitter", C.POINTER(C.c_int32)), ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
                ("n_emitters", C.c_uint32), ("emitters", C.POINTER(Emitter)), ("camera", Camera), ("environment", C.POINTER(C.c_float)),
                ("n_rtrans", C.c_uint32), ("rtrans_samples", C.c_uint32), ("rtrans", C.POINTER(C.c_float)),
                ("n_spheres", C.c_uint32), ("spheres", C.POINTER(Sphere)), ("envmap", C.POINTER(EnvMap)),
                ("texcoords", C.POINTER(C.c_float)), ("n_textures", C.c_uint32), ("textures", C.POINTER(Texture))]


class _StatsMixin:
    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PassStats(C.Structure, _StatsMixin):
    _fields_ = [("seconds", C.c_double), ("passes_rendered_total", C.c_int32), ("passes_rendered_local", C.c_int32),
                ("variance", C.c_float), ("samples", C.c_uint64), ("rays", C.c_uint64), ("path_length_sum", C.c_uint64),
                ("vertices_committed", C.c_uint64)]


class TreeStats(C.Structure, _StatsMixin):
    _fields_ = [("min_depth", C.c_int32), ("max_depth", C.c_int32), ("avg_depth", C.c_float),
                ("min_mean_radiance", C.c_float), ("avg_mean_radiance", C.c_float), ("max_mean_radiance", C.c_float),
                ("min_nodes", C.c_uint64), ("max_nodes", C.c_uint64), ("avg_nodes", C.c_float),
                ("min_stat_weight", C.c_float), ("avg_stat_weight", C.c_float), ("max_stat_weight", C.c_float),
                ("n_leaves", C.c_uint32), ("n_stree_nodes", C.c_uint32), ("n_dtree_nodes", C.c_uint64)]


class SDTreeInfo(C.Structure):
    _fields_ = [("n_stree_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("n_sampling_nodes", C.c_uint64),
                ("n_building_nodes", C.c_uint64), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("iter", C.c_int32), ("is_built", C.c_int32)]


class SDTreeLoad(C.Structure):
    """ppg_sdtree_load (include/ppg.h)"""
    _fields_ = [("iter", C.c_int32), ("passes_rendered", C.c_int32), ("_reserved", C.c_int32 * 2)]


def read_sdt(path):
    """An .sdt dump (ppg_dump_sdtree / dumpSDTree, the reference's DTreeWrapper::dump, GP:699-711) as numpy arrays — no GPU, no library; for
    inspection and tests.  Returns {"camera": float32 [4, 4], "leaves": [...]}, the leaves in file order (depth first, child 0 before child
    1; leaves of statistical weight 0 are not in the file), each a dict: p, size (float32 [3]), mean (float32), weight (int), num_nodes,
    node_sums (float32 [n, 4]) and node_children (uint16 [n, 4]).  Only the framing is checked here (ValueError for a truncated file): what
    the engine refuses beyond that is Engine.load_sdtree's business."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 64:
        raise ValueError("%s: truncated: %d bytes, the camera matrix alone takes 64" % (path, len(data)))
    node = np.dtype([("sum", "<f4"), ("child", "<u2")])
    out = {"camera": np.frombuffer(data, "<f4", 16).reshape(4, 4).copy(), "leaves": []}
    off = 64
    while off < len(data):
        if len(data) - off < 44:
            raise ValueError("%s: leaf %d at offset %d: truncated: %d trailing bytes do not form a leaf" % (path, len(out["leaves"]), off, len(data) - off))
        head = np.frombuffer(data, "<f4", 7, off)
        weight, n = (int(v) for v in np.frombuffer(data, "<u8", 2, off + 28))
        if n * 24 > len(data) - off - 44:
            raise ValueError("%s: leaf %d at offset %d: truncated: numNodes %d needs more than the %d bytes that remain"
                             % (path, len(out["leaves"]), off, n, len(data) - off - 44))
        nodes = np.frombuffer(data, node, 4 * n, off + 44).reshape(n, 4)
        out["leaves"].append({"offset": off, "p": head[0:3].copy(), "size": head[3:6].copy(), "mean": np.float32(head[6]), "weight": weight,
                              "num_nodes": n, "node_sums": np.ascontiguousarray(nodes["sum"]), "node_children": np.ascontiguousarray(nodes["child"])})
        off += 44 + 24 * n
    return out


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("launches", C.c_uint64), ("units", C.c_uint64)]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Engine:
    """One integrator context (ppg_ctx).  Methods are 1:1 with include/ppg.h."""

    def __init__(self, lib, prefix="ppg_", **props):
        if isinstance(lib, str):
            if not os.path.exists(lib):
                raise FileNotFoundError(
                    "%s not found — build it with `python __graft_entry__.py` (no CPU fallback exists)" % lib)
            lib = C.CDLL(lib)
        self.lib, self.prefix = lib, prefix
        self.cfg = Config.make(**props)
        self.props = dict(Config.DEFAULTS, **props)
        self.ctx = C.c_void_p()
        self._f("last_error").restype = C.c_char_p
        self._f("last_error").argtypes = [C.c_void_p]
        rc = self._f("create")(C.byref(self.cfg), C.byref(self.ctx))
        if rc != 0:
            raise PPGError(rc, (self._f("last_error")(None) or b"").decode())
        self._scene_keep = None
        self.width = self.height = 0

    @classmethod
    def hip(cls, **props):
        # If the process is going to use torch.distributed (RCCL) it must import torch *before* this call:
        # torch ships its own HIP runtime and only one runtime per process can own the GPUs.
        return cls(hip_library_path(), "ppg_", **props)

    def _f(self, name):
        return getattr(self.lib, self.prefix + name)

    def _call(self, name, *args):
        rc = self._f(name)(self.ctx, *args)
        if rc != 0:
            raise PPGError(rc, (self._f("last_error")(self.ctx) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "ctx", None):
            f = self._f("destroy")
            f.restype = None
            f(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scene -------------------------------------------------------------------------------
    def set_scene(self, desc):
        if has_media(desc) and self.prefix != "ppg_":
            raise NotImplementedError("%s: participating media are not implemented here" % self.prefix)
        if has_blends(desc):  # children stated as dicts join the material list
            if self.prefix != "ppg_":
                raise NotImplementedError("%s: the blendbsdf / mixturebsdf combinators are not implemented here" % self.prefix)
            import copy
            desc = copy.copy(desc)
            desc.materials = expand_blends(desc.materials)
        if self.prefix != "ppg_" and any(Material.from_dict(m).type in Material.LOBES for m in desc.materials):
            raise NotImplementedError("%s: roughdiffuse, difftrans and phong are not implemented here" % self.prefix)
        if self.prefix != "ppg_" and any(m.get("normal_map") is not None or Material.from_dict(m).type == Material.NULL for m in desc.materials):
            raise NotImplementedError("%s: the normalmap adapter and the null BSDF are not implemented here" % self.prefix)
        s = Scene()
        pos = np.ascontiguousarray(desc.positions, np.float32)
        idx = np.ascontiguousarray(desc.indices, np.uint32)
        tm = np.ascontiguousarray(desc.tri_material, np.uint32)
        te = np.ascontiguousarray(desc.tri_emitter, np.int32)
        nrm = None if desc.normals is None else np.ascontiguousarray(desc.normals, np.float32)
        mats = (Material * len(desc.materials))()
        for i, m in enumerate(desc.materials):
            mats[i] = Material.from_dict(m)
        ems = (Emitter * max(1, len(desc.emitters)))()
        for i, e in enumerate(desc.emitters):
            ems[i].radiance[:] = [float(v) for v in e["radiance"]]
        s.n_vertices, s.positions = pos.shape[0], _fp(pos)
        if nrm is not None:
            s.normals = _fp(nrm)
        s.n_triangles, s.indices = idx.shape[0], _p(idx, C.c_uint32)
        s.tri_material = _p(tm, C.c_uint32)
        s.tri_emitter = _p(te, C.c_int32)
        s.n_materials, s.materials = len(desc.materials), mats
        s.n_emitters, s.emitters = len(desc.emitters), ems
        env = getattr(desc, "environment", None)
        if env is not None:
            env_arr = (C.c_float * 3)(*[float(v) for v in env])
            s.environment = C.cast(env_arr, C.POINTER(C.c_float))
        rt = getattr(desc, "rtrans", None)
        if rt is not None and len(rt):
            rt = np.ascontiguousarray(rt, np.float32)
            s.n_rtrans, s.rtrans_samples, s.rtrans = rt.shape[0], rt.shape[1] - 1, _fp(rt)
        sph = getattr(desc, "spheres", None) or []
        sph_arr = (Sphere * max(1, len(sph)))()
        for i, d in enumerate(sph):
            sph_arr[i] = Sphere.from_dict(d)
        if sph:
            s.n_spheres, s.spheres = len(sph), sph_arr
        envmap = None
        if getattr(desc, "envmap", None) is not None:
            envmap = EnvMap.from_dict(desc.envmap)
            s.envmap = C.pointer(envmap)
        uvs = getattr(desc, "texcoords", None)
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, np.float32)
            assert uvs.shape == (pos.shape[0], 2)
            s.texcoords = _fp(uvs)
        texs = getattr(desc, "textures", None) or []
        tex_arr = (Texture * max(1, len(texs)))()
        tex_keep = []
        for i, d in enumerate(texs):
            t = Texture.from_dict(d)
            tex_keep.append(t._keep)
            tex_arr[i] = t
        if texs:
            s.n_textures, s.textures = len(texs), tex_arr
        cam = desc.camera
        s.camera.sample_to_camera[:] = [float(v) for v in np.asarray(cam["sample_to_camera"], np.float32).reshape(-1)]
        s.camera.camera_to_world[:] = [float(v) for v in np.asarray(cam["camera_to_world"], np.float32).reshape(-1)]
        s.camera.near_clip, s.camera.far_clip = cam["near_clip"], cam["far_clip"]
        s.camera.width, s.camera.height = cam["width"], cam["height"]
        self._scene_keep = (pos, idx, tm, te, nrm, mats, ems, rt, sph_arr, envmap, uvs, tex_arr, tex_keep)
        self._send_side_lists(self._BEFORE_SET_SCENE, desc)
        if self.prefix == "ppg_" and (has_media(desc) or getattr(self, "_media", False)):  # (or to clear what an earlier description left)
            self.set_media(getattr(desc, "media", None), getattr(desc, "tri_media", None), getattr(desc, "sphere_media", None),
                           getattr(desc, "shape_media", None), getattr(desc, "camera_medium", 0))
        try:
            self._call("set_scene", C.byref(s))
        except PPGError:
            # a refused scene leaves the previous one set: its media list must not stay behind in the context, where a later
            # ppg_set_scene of another description would consume it
            if getattr(self, "_media", False):
                self.set_media([])
            raise
        self.width, self.height = cam["width"], cam["height"]
        self._send_side_lists(self._AFTER_SET_SCENE, desc)

    # What set_scene sends beside the scene itself: (setter, whether the description carries it, what to send, the attribute that remembers
    # what the context holds — None: always sent —, what a library other than ppg_ says to a description that carries it — None: nothing left to say).  The lists go
    # first, ppg_set_scene consumes the context's: shapes and the per-material lists are always sent — one entry per material, or the empty
    # list that clears the context's; a description may also state `coatings` / `blends` itself, as records or dicts.  Delta emitters, the
    # film filter and the lens are sent for a description that has one, or to reset what an earlier one left: a context that never had one
    # is left alone.
    _BEFORE_SET_SCENE = (
        ("set_delta_emitters", lambda d: bool(getattr(d, "delta_emitters", None)), lambda d: getattr(d, "delta_emitters", None) or [], "_delta",
         "point, spot and directional emitters are not implemented here"),
        ("set_shapes", lambda d: bool(getattr(d, "shapes", None)), lambda d: getattr(d, "shapes", None) or [], None,
         "analytic disks and cylinders are not implemented here"),
        ("set_material_textures", has_parameter_textures, lambda d: d.materials if has_parameter_textures(d) else [], None,
         "bitmaps on specular / alpha / opacity (specular_texture, alpha_texture, opacity_texture) are not implemented here"),
        ("set_microfacet", has_general_microfacet, lambda d: d.materials if has_general_microfacet(d) else [], None,
         "alpha_v, distribution = phong and sample_visible = False are not implemented here"),
        ("set_coatings", has_coatings, lambda d: d.coatings if getattr(d, "coatings", None) is not None else (d.materials if has_coatings(d) else []), None,
         "the coating / roughcoating adapters are not implemented here"),
        ("set_blends", has_blends, lambda d: d.blends if getattr(d, "blends", None) is not None else (d.materials if has_blends(d) else []), None,
         None),  # (set_scene has refused a blend for another library before it expanded the children)
    )
    _AFTER_SET_SCENE = (
        ("set_rfilter", lambda d: getattr(d, "rfilter", None) is not None, lambda d: getattr(d, "rfilter", None), "_rfilter",
         "reconstruction filters other than the default box are not implemented here"),
        ("set_lens", lambda d: getattr(d, "lens", None) is not None, lambda d: getattr(d, "lens", None), "_lens",
         "the thin-lens camera is not implemented here"),
    )

    def _send_side_lists(self, rows, desc):
        for setter, carries, items, remembered, refusal in rows:
            if self.prefix != "ppg_":
                if refusal and carries(desc):
                    raise NotImplementedError("%s: %s" % (self.prefix, refusal))
            elif remembered is None or carries(desc) or getattr(self, remembered, None):
                getattr(self, setter)(items(desc))

    def _set_list(self, name, cls, items):
        """ppg_set_<name>(array, n): `items` are records of `cls` or what cls.from_dict takes"""
        items = list(items or [])
        arr = (cls * max(1, len(items)))()
        for i, d in enumerate(items):
            arr[i] = d if isinstance(d, cls) else cls.from_dict(d)
        self._call("set_" + name, arr, C.c_uint32(len(items)))
        return items

    def set_delta_emitters(self, emitters):
        """ppg_set_delta_emitters: a list of emitter dicts (DeltaEmitter); an empty list clears it.  Takes effect at the next set_scene."""
        self._delta = self._set_list("delta_emitters", DeltaEmitter, emitters)

    def set_media(self, media, tri_media=None, sphere_media=None, shape_media=None, camera_medium=0):
        """ppg_set_media: a list of medium dicts (Medium), the binding words per triangle / sphere / shape (media_word; None: none) and the
        sensor's medium (1 + index, 0: none); an empty list clears it.  Heterogeneous media among them send their volumes first
        (set_media_volumes).  Takes effect at, and is validated by, the next set_scene."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: participating media are not implemented here" % self.prefix)
        media = list(media or [])
        volumes, entries, keep_volumes = flatten_media_volumes(media)  # heterogeneous media: their volumes go first
        if entries or getattr(self, "_media_volumes", False):
            self.set_media_volumes(volumes, entries)
        m = Media()
        arr = (Medium * max(1, len(media)))()
        for i, d in enumerate(media):
            arr[i] = d if isinstance(d, Medium) else Medium.from_dict(d)
        m.n_media, m.media, m.camera_medium = len(media), arr, int(camera_medium)
        keep = [arr]
        for name, words in (("tri_media", tri_media), ("sphere_media", sphere_media), ("shape_media", shape_media)):
            if words is None:
                continue
            w = np.ascontiguousarray(words, np.uint32).reshape(-1)
            w = w if w.size else np.zeros(1, np.uint32)  # (an array of no entries is still an array)
            keep.append(w)
            setattr(m, "n_" + name, int(np.asarray(words).size))
            setattr(m, name, _p(w, C.c_uint32))
        self._call("set_media", C.byref(m))
        self._media = bool(media)

    def set_media_volumes(self, volumes, entries):
        """ppg_set_media_volumes: Volume and MediumVolumes records (flatten_media_volumes makes them of medium dicts; set_media calls this
        itself); no entries clear the list.  Takes effect at, and is validated by, the next set_scene."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: participating media are not implemented here" % self.prefix)
        volumes, entries = list(volumes or []), list(entries or [])
        v = MediaVolumes()
        varr, earr = (Volume * max(1, len(volumes)))(*volumes), (MediumVolumes * max(1, len(entries)))(*entries)
        v.n_volumes, v.n_entries, v.volumes, v.entries = len(volumes), len(entries), varr, earr
        self._call("set_media_volumes", C.byref(v))
        self._media_volumes = bool(entries)

    def _debug_items(self, name, items, item_dtype, out_dtype, item_cls, out_cls):
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: ppg_%s is not implemented here" % (self.prefix, name))
        items = np.ascontiguousarray(items, item_dtype).reshape(-1)
        out = np.zeros(items.shape[0], out_dtype)
        assert out.itemsize == C.sizeof(out_cls) and items.itemsize == C.sizeof(item_cls)
        self._call(name, C.c_uint32(items.shape[0]), items.ctypes.data_as(C.POINTER(item_cls)), out.ctypes.data_as(C.POINTER(out_cls)))
        return out

    def debug_volume(self, items):
        """ppg_debug_volume (include/ppg_testhooks.h): items a structured array (DEBUG_VOLUME_ITEM_DTYPE) through the hetmedia family's
        volume lookups; a structured array (DEBUG_VOLUME_OUT_DTYPE)."""
        return self._debug_items("debug_volume", items, DEBUG_VOLUME_ITEM_DTYPE, DEBUG_VOLUME_OUT_DTYPE, DebugVolumeItem, DebugVolumeOut)

    def debug_hetmedium(self, items):
        """ppg_debug_hetmedium (include/ppg_testhooks.h): items a structured array (DEBUG_HETMEDIUM_ITEM_DTYPE) through the hetmedia
        family's sampleDistance and evalTransmittance; a structured array (DEBUG_HETMEDIUM_OUT_DTYPE)."""
        return self._debug_items("debug_hetmedium", items, DEBUG_HETMEDIUM_ITEM_DTYPE, DEBUG_HETMEDIUM_OUT_DTYPE, DebugHetmediumItem, DebugHetmediumOut)

    def debug_medium(self, items):
        """ppg_debug_medium (include/ppg_testhooks.h): items a structured array (DEBUG_MEDIUM_ITEM_DTYPE) through the media family's
        sampleDistance / evalTransmittance / phase sample and eval; a structured array (DEBUG_MEDIUM_OUT_DTYPE)."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: ppg_debug_medium is not implemented here" % self.prefix)
        items = np.ascontiguousarray(items, DEBUG_MEDIUM_ITEM_DTYPE).reshape(-1)
        out = np.zeros(items.shape[0], DEBUG_MEDIUM_OUT_DTYPE)
        assert out.itemsize == C.sizeof(DebugMediumOut) and items.itemsize == C.sizeof(DebugMediumItem)
        self._call("debug_medium", C.c_uint32(items.shape[0]), items.ctypes.data_as(C.POINTER(DebugMediumItem)), out.ctypes.data_as(C.POINTER(DebugMediumOut)))
        return out

    def set_shapes(self, shapes):
        """ppg_set_shapes: a list of shape dicts (Shape); an empty list clears it.  Takes effect at, and is validated by, the next set_scene."""
        self._set_list("shapes", Shape, shapes)

    def debug_intersect(self, rays, any_hit=False):
        """ppg_debug_intersect (include/ppg_testhooks.h): rays float32 [n, 8] = (o, mint, d, maxt) through the scene's closest-hit (or
        any-hit) trace and intersection record; a structured array (DEBUG_HIT_DTYPE)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], DEBUG_HIT_DTYPE)
        assert out.itemsize == C.sizeof(DebugHit)
        self._call("debug_intersect", C.c_uint32(rays.shape[0]), _fp(rays), out.ctypes.data_as(C.POINTER(DebugHit)), C.c_int32(1 if any_hit else 0))
        return out

    def debug_shading_frame(self, rays):
        """ppg_debug_shading_frame (include/ppg_testhooks.h): rays float32 [n, 8] = (o, mint, d, maxt) to their closest hit and the shading
        frame there, before and after the bumpmap / normalmap adapter; a structured array (DEBUG_FRAME_DTYPE)."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: ppg_debug_shading_frame is not implemented here" % self.prefix)
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], DEBUG_FRAME_DTYPE)
        assert out.itemsize == C.sizeof(DebugFrame)
        self._call("debug_shading_frame", C.c_uint32(rays.shape[0]), _fp(rays), out.ctypes.data_as(C.POINTER(DebugFrame)))
        return out

    def debug_camera_rays(self, first_sample=0, n_samples=1):
        """ppg_debug_camera_rays (include/ppg_testhooks.h): the camera rays of the whole film for the sample indices first_sample ..
        first_sample + n_samples - 1, float32 [n_samples, height * width, 8] = (o, mint, d, maxt): what debug_intersect takes."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: ppg_debug_camera_rays is not implemented here" % self.prefix)
        out = np.zeros((int(n_samples), self.height * self.width, 8), np.float32)
        self._call("debug_camera_rays", C.c_uint32(int(first_sample)), C.c_uint32(int(n_samples)), _fp(out))
        return out

    def render_field_planes(self, fields, spp=1, undefined=None, first_sample=0):
        """ppg_render_fields (include/ppg.h): `fields` = Mitsuba's field names (FIELD_NAMES; repeats allowed), `undefined` = per field the
        value of a sample whose ray leaves the scene (a number or an rgb triple; None: 0) -> float32 [len(fields), height, width, 3]."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: ppg_render_fields is not implemented here" % self.prefix)
        fields = list(fields)
        codes = [field_code(name) for name in fields]
        f = Fields()
        f.n_fields, f.spp, f.first_sample = len(fields), int(spp), int(first_sample)
        undefined = list(undefined) if undefined is not None else [0.0] * len(fields)
        if len(undefined) != len(fields):
            raise ValueError("undefined: one value per field")
        for k in range(min(len(fields), MAX_FIELDS)):
            f.field[k] = codes[k]
            f.undefined[k][:] = [float(v) for v in np.broadcast_to(np.asarray(undefined[k], np.float32), (3,))]
        out = np.zeros((max(1, min(len(fields), MAX_FIELDS)), self.height, self.width, 3), np.float32)
        self._call("render_fields", C.byref(f), _fp(out))
        return out

    def render_fields(self, fields, spp=1, undefined=None, first_sample=0):
        """The feature buffers of the first hit as a dict from field name to a float32 array [height, width, 3] (render_field_planes)."""
        fields = list(fields)
        planes = self.render_field_planes(fields, spp, undefined, first_sample)
        return {name: planes[k] for k, name in enumerate(fields)}

    DEBUG_TRACE_MODES = dict(lane=0, lane_any=1, lane_vote=2, resume=3, wave=4, ktrace=5)

    def debug_intersect_mode(self, rays, mode, param=0):
        """ppg_debug_intersect_mode (include/ppg_testhooks.h): the rays through another form of the closest-hit traversal — mode is a key of
        DEBUG_TRACE_MODES — -> (structured array (DEBUG_HIT_DTYPE), stats uint32 [4])."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], DEBUG_HIT_DTYPE)
        stats = np.zeros(4, np.uint32)
        self._call("debug_intersect_mode", C.c_uint32(rays.shape[0]), _fp(rays), out.ctypes.data_as(C.POINTER(DebugHit)),
                   C.c_int32(self.DEBUG_TRACE_MODES[mode]), C.c_int32(int(param)), stats.ctypes.data_as(C.POINTER(C.c_uint32)))
        return out, stats

    def debug_sample_direct(self, ref, ref_n, u):
        """ppg_debug_sample_direct: emitter_sample_direct per (ref [n, 3], ref_n [n, 3], u [n, 2]); a structured array (DEBUG_DIRECT_DTYPE)."""
        ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3)
        ref_n = np.ascontiguousarray(ref_n, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        assert ref.shape[0] == ref_n.shape[0] == u.shape[0]
        out = np.zeros(ref.shape[0], DEBUG_DIRECT_DTYPE)
        assert out.itemsize == C.sizeof(DebugDirect)
        self._call("debug_sample_direct", C.c_uint32(ref.shape[0]), _fp(ref), _fp(ref_n), _fp(u), out.ctypes.data_as(C.POINTER(DebugDirect)))
        return out

    def debug_sample_direct_as(self, ref, ref_n, u, family=-1, full=1):
        """ppg_debug_sample_direct_as: emitter_sample_direct<full> of kernel family `family` (-1: what a render of the scene would run); on the
        oracle ppgo_debug_sample_direct, which has no such selectors.  Arrays as debug_sample_direct; a structured array (DEBUG_DIRECT_EX_DTYPE)."""
        ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3)
        ref_n = np.ascontiguousarray(ref_n, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 2)
        assert ref.shape[0] == ref_n.shape[0] == u.shape[0]
        out = np.zeros(ref.shape[0], DEBUG_DIRECT_EX_DTYPE)
        assert out.itemsize == C.sizeof(DebugDirectEx)
        args = (C.c_uint32(ref.shape[0]), _fp(ref), _fp(ref_n), _fp(u), out.ctypes.data_as(C.POINTER(DebugDirectEx)))
        if self.prefix == "ppg_":
            self._call("debug_sample_direct_as", C.c_int32(int(family)), C.c_int32(int(full)), *args)
        else:
            self._call("debug_sample_direct", *args)
        return out

    def debug_pdf_direct(self, rays, ref_n, family=-1):
        """ppg_debug_pdf_direct / ppgo_debug_pdf_direct: per ray (float32 [n, 8] = (o, mint, d, maxt)) and normal of the vertex it left (ref_n
        [n, 3], zeros = none) the emitter it finds and the density next-event estimation has for it; a structured array (DEBUG_PDF_DTYPE)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        ref_n = np.ascontiguousarray(ref_n, np.float32).reshape(-1, 3)
        assert rays.shape[0] == ref_n.shape[0]
        out = np.zeros(rays.shape[0], DEBUG_PDF_DTYPE)
        assert out.itemsize == C.sizeof(DebugPdf)
        args = (C.c_uint32(rays.shape[0]), _fp(rays), _fp(ref_n), out.ctypes.data_as(C.POINTER(DebugPdf)))
        if self.prefix == "ppg_":
            self._call("debug_pdf_direct", C.c_int32(int(family)), *args)
        else:
            self._call("debug_pdf_direct", *args)
        return out

    DEBUG_COMMIT_ROUTES = dict(commit=0, commit_split=1, records=2, records_split=3)

    def debug_commit(self, route, nv, key, dim, p, d, radiance, throughput, bsdf_val, wo_pdf, bsdf_pdf, dtree_pdf, is_delta, late=None,
                     n_vertices=None, records_cap=None):
        """ppg_debug_commit / ppgo_debug_commit (include/ppg_testhooks.h): explicit vertices through the commit of a batch and the round's
        end.  Per path nv, key, dim (uint32 [n]) and late (bool [n] or None); per vertex, path after path, p, d, radiance, throughput,
        bsdf_val (float32 [m, 3]), wo_pdf, bsdf_pdf, dtree_pdf (float32 [m]) and is_delta (bool [m]).  -> dict(committed, keys uint64 [k],
        records (ADAM_RECORD_DTYPE) in key order, adam_state uint32 [n_stree_nodes, 6]).  n_vertices: what to claim instead of len(wo_pdf); records_cap:
        room for the keys and records (default 64 per vertex)."""
        u32 = lambda a: np.ascontiguousarray(a, np.uint32).reshape(-1)
        f3 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 3)
        f1 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1)
        nv, key, dim = u32(nv), u32(key), u32(dim)
        p, d, radiance, throughput, bsdf_val = f3(p), f3(d), f3(radiance), f3(throughput), f3(bsdf_val)
        wo_pdf, bsdf_pdf, dtree_pdf = f1(wo_pdf), f1(bsdf_pdf), f1(dtree_pdf)
        is_delta = np.ascontiguousarray(is_delta, np.uint8).reshape(-1)
        m = wo_pdf.shape[0]
        assert key.shape[0] == nv.shape[0] == dim.shape[0]
        assert all(a.shape[0] == m for a in (p, d, radiance, throughput, bsdf_val, bsdf_pdf, dtree_pdf, is_delta))
        late8 = None if late is None else np.ascontiguousarray(late, np.uint8).reshape(-1)
        assert late8 is None or late8.shape[0] == nv.shape[0]
        arg = DebugCommitIn()
        arg.route = self.DEBUG_COMMIT_ROUTES[route] if isinstance(route, str) else int(route)
        arg.n_paths = nv.shape[0]
        arg.n_vertices = m if n_vertices is None else int(n_vertices)
        arg.nv, arg.key, arg.dim = _p(nv, C.c_uint32), _p(key, C.c_uint32), _p(dim, C.c_uint32)
        arg.late = None if late8 is None else _p(late8, C.c_uint8)
        arg.p, arg.d, arg.radiance, arg.throughput, arg.bsdf_val = _fp(p), _fp(d), _fp(radiance), _fp(throughput), _fp(bsdf_val)
        arg.wo_pdf, arg.bsdf_pdf, arg.dtree_pdf, arg.is_delta = _fp(wo_pdf), _fp(bsdf_pdf), _fp(dtree_pdf), _p(is_delta, C.c_uint8)
        n_nodes = int(self.sdtree_info().n_stree_nodes)
        state = np.zeros((n_nodes, 6), np.uint32)
        cap = int(records_cap) if records_cap is not None else 64 * m + 64  # (the box spatial filter: a record per leaf a voxel overlaps)
        keys = np.zeros(cap, np.uint64)
        recs = np.zeros(cap, ADAM_RECORD_DTYPE)
        out = DebugCommitOut()
        out.keys_cap = out.records_cap = cap
        out.keys, out.records, out.adam_state = _p(keys, C.c_uint64), recs.ctypes.data_as(C.c_void_p), _p(state, C.c_uint32)
        self._call("debug_commit", C.byref(arg), C.byref(out))
        if max(out.n_keys, out.n_records) > cap:  # (the call has been applied; what did not fit was counted only)
            raise PPGError(-5, "debug_commit: %d records exceed records_cap = %d" % (max(out.n_keys, out.n_records), cap))
        return dict(committed=int(out.committed), keys=keys[:out.n_keys].copy(), records=recs[:out.n_records].copy(), adam_state=state)

    def set_material_textures(self, slots):
        """ppg_set_material_textures: one entry per material — a material dict (its specular_texture / alpha_texture / opacity_texture keys) or
        a MaterialTextures; an empty list clears it.  Takes effect at the next set_scene."""
        self._set_list("material_textures", MaterialTextures, slots)

    def set_microfacet(self, entries):
        """ppg_set_microfacet: one entry per material — a material dict (its alpha_v / alpha_v_texture / distribution / sample_visible keys) or
        a Microfacet; an empty list clears it.  Takes effect at, and is validated by, the next set_scene."""
        self._set_list("microfacet", Microfacet, entries)

    def set_coatings(self, entries):
        """ppg_set_coatings: one entry per material — a material dict (its `coating` key), a coating dict or a Coating; an empty list clears
        it.  Takes effect at, and is validated by, the next set_scene."""
        self._set_list("coatings", Coating, entries)

    def set_blends(self, entries):
        """ppg_set_blends: one entry per material — a material dict (its `blend` key, children as indices), a blend dict or a Blend; an empty
        list clears it.  Takes effect at, and is validated by, the next set_scene."""
        self._set_list("blends", Blend, entries)

    def debug_bsdf(self, material, wi, wo, sample, key=None, uv=None):
        """ppg_debug_bsdf (include/ppg_testhooks.h): the render's mat_eval / mat_pdf / mat_sample on material(s) `material` of the scene, per
        item local wi, wo [n, 3], the 2-D sample [n, 2], the sampler key of roughdielectric's extra draw and the hit's uv; a structured
        array (DEBUG_BSDF_OUT_DTYPE)."""
        wo = np.ascontiguousarray(wo, np.float32).reshape(-1, 3)
        n = wo.shape[0]
        items = np.zeros(n, DEBUG_BSDF_ITEM_DTYPE)
        items["material"] = material
        items["wi"] = np.broadcast_to(np.asarray(wi, np.float32), (n, 3))
        items["wo"] = wo
        items["sample"] = np.broadcast_to(np.asarray(sample, np.float32), (n, 2))
        items["key"] = 0 if key is None else key
        items["uv"] = 0.0 if uv is None else np.broadcast_to(np.asarray(uv, np.float32), (n, 2))
        out = np.zeros(n, DEBUG_BSDF_OUT_DTYPE)
        assert items.itemsize == C.sizeof(DebugBsdfItem) and out.itemsize == C.sizeof(DebugBsdfOut)
        self._call("debug_bsdf", C.c_uint32(n), items.ctypes.data_as(C.POINTER(DebugBsdfItem)), out.ctypes.data_as(C.POINTER(DebugBsdfOut)))
        return out

    DEBUG_BSDF_UNITS = {"FULL": 0, "LEAN": 1, "COMMON": 2}

    def debug_bsdf_as(self, items, family=-1, unit="FULL"):
        """ppg_debug_bsdf_as (include/ppg_testhooks.h): `items` (a DEBUG_BSDF_ITEM_DTYPE array, in one launch) through the BSDF layer as kernel
        family `family` (-1: what a render of the scene would run) and unit FULL / LEAN / COMMON compiled it; a structured array
        (DEBUG_BSDF_OUT_DTYPE) whose _pad[0] carries the smooth / backside-or-transmission / has-null bits."""
        items = np.ascontiguousarray(items, DEBUG_BSDF_ITEM_DTYPE)
        out = np.zeros(len(items), DEBUG_BSDF_OUT_DTYPE)
        assert items.itemsize == C.sizeof(DebugBsdfItem) and out.itemsize == C.sizeof(DebugBsdfOut)
        self._call("debug_bsdf_as", C.c_int32(int(family)), C.c_int32(int(self.DEBUG_BSDF_UNITS.get(unit, unit))), C.c_uint32(len(items)),
                   items.ctypes.data_as(C.POINTER(DebugBsdfItem)), out.ctypes.data_as(C.POINTER(DebugBsdfOut)))
        return out

    def debug_math_eval(self, family, via, op, a, b=None):
        """ppg_debug_math_eval (include/ppg_testhooks.h): op of include/ppg_mathcheck.h on the bit patterns a, b (float32 or uint32 arrays),
        in kernel family `family`'s module (-1: the library's host code), via 0 the header's functions or 1 the module's dm_ copies.
        -> (out0, out1) uint32; an element outside the op's domain stays 0."""
        def bits(v):
            v = np.ascontiguousarray(v)
            return np.ascontiguousarray(v.view(np.uint32) if v.dtype == np.float32 else v.astype(np.uint32, casting="same_kind")).ravel()
        a = bits(a)
        b = np.zeros_like(a) if b is None else bits(b)
        assert a.size == b.size
        o0, o1 = np.zeros_like(a), np.zeros_like(a)
        up = C.POINTER(C.c_uint32)
        self._call("debug_math_eval", C.c_int32(family), C.c_int32(via), C.c_int32(op), C.c_uint32(a.size), a.ctypes.data_as(up), b.ctypes.data_as(up),
                   o0.ctypes.data_as(up), o1.ctypes.data_as(up))
        return o0, o1

    def debug_math_checksum(self, family, via, op, first_block=0, n_blocks=256):
        """ppg_debug_math_checksum: the checksums of blocks first_block .. first_block + n_blocks - 1 of the float patterns under a
        one-argument op; uint64 [n_blocks]."""
        out = np.zeros(n_blocks, np.uint64)
        self._call("debug_math_checksum", C.c_int32(family), C.c_int32(via), C.c_int32(op), C.c_uint32(first_block), C.c_uint32(n_blocks),
                   out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def set_lens(self, lens):
        """ppg_set_lens: lens = {"aperture_radius", "focus_distance"} (Lens) or None for the pinhole"""
        self._lens = None if lens is None else Lens.from_dict(lens)
        self._call("set_lens", None if self._lens is None else C.byref(self._lens))

    def set_rfilter(self, rfilter):
        """ppg_set_rfilter: rfilter = a filter dict (RFilter) or None for the default box"""
        self._rfilter = RFilter.from_dict(rfilter)
        self._call("set_rfilter", C.byref(self._rfilter))

    def set_shard(self, rank, world, tile_size=32):
        self._call("set_shard", C.c_int32(rank), C.c_int32(world), C.c_int32(tile_size))

    # -- rendering ---------------------------------------------------------------------------
    def render(self):
        self._call("render")

    def begin_render(self):
        self._call("begin_render")

    def begin_iteration(self, is_final):
        self._call("begin_iteration", C.c_int32(int(is_final)))

    def set_final(self, is_final):
        self._call("set_final", C.c_int32(int(is_final)))

    def set_adam_regions(self, regions):
        """Rounds by image region (include/ppg.h ppg_set_adam_regions): 0 = off (default), R >= 2 = R rounds per pass in the early iterations."""
        self._call("set_adam_regions", C.c_int32(int(regions)))

    def set_do_nee(self, v):
        self._call("set_do_nee", C.c_int32(int(v)))

    def render_passes(self, n):
        st = PassStats()
        self._call("render_passes", C.c_int32(n), C.byref(st))
        return st

    def render_passes_nostat(self, n):
        self._call("render_passes_nostat", C.c_int32(n))

    def finish_passes(self):
        st = PassStats()
        self._call("finish_passes", C.byref(st))
        return st

    def build_sdtree(self):
        st = TreeStats()
        self._call("build_sdtree", C.byref(st))
        return st

    def end_iteration(self):
        self._call("end_iteration")

    def end_render(self):
        self._call("end_render")

    def cancel(self):
        self._call("cancel")

    def read_film(self):
        out = np.empty((self.height, self.width, 3), np.float32)
        self._call("read_film", _fp(out))
        return out

    def read_variance(self):
        out = np.empty((self.height, self.width, 3), np.float32)
        self._call("read_variance", _fp(out))
        return out

    def dump_sdtree(self, path):
        self._call("dump_sdtree", path.encode())

    def load_sdtree(self, path, iter=0, passes_rendered=0):
        """ppg_load_sdtree (include/ppg.h "Loading a dumped SD-tree"): after begin_render(), with no iteration open.  iter and passes_rendered
        are sdtree_info().iter and the passes_rendered_total of the context that dumped the file.  HIP library only."""
        if self.prefix != "ppg_":
            raise NotImplementedError("%s: loading a dumped SD-tree is not implemented here" % self.prefix)
        opts = SDTreeLoad(int(iter), int(passes_rendered))
        self._call("load_sdtree", os.fsencode(path), C.byref(opts))

    # -- SD-tree access ----------------------------------------------------------------------
    def sdtree_info(self):
        info = SDTreeInfo()
        self._call("sdtree_info_get", C.byref(info))
        return info

    def read_sdtree(self):
        """The S-tree and both D-tree sets in the reference's node numbering (dict of numpy arrays)."""
        info = self.sdtree_info()
        n = info.n_stree_nodes
        axis = np.zeros(n, np.int32)
        children = np.zeros((n, 2), np.uint32)
        self._call("sdtree_read_stree", _p(axis, C.c_int32), _p(children, C.c_uint32))
        out = {"axis": axis, "children": children, "n_leaves": info.n_leaves, "iter": info.iter,
               "aabb_min": np.array(info.aabb_min[:], np.float32), "aabb_max": np.array(info.aabb_max[:], np.float32)}
        for which, name, total in ((0, "sampling", info.n_sampling_nodes), (1, "building", info.n_building_nodes)):
            off = np.zeros(n, np.uint64)
            nn = np.zeros(n, np.uint32)
            md = np.zeros(n, np.int32)
            sm = np.zeros(n, np.float32)
            sw = np.zeros(n, np.float64)
            self._call("sdtree_read_dtree_headers", C.c_int32(which), _p(off, C.c_uint64), _p(nn, C.c_uint32),
                       _p(md, C.c_int32), _fp(sm), _p(sw, C.c_double))
            total = int(total)
            sums = np.zeros((total, 4), np.float32)
            ch = np.zeros((total, 4), np.uint16)
            fx = np.zeros((total, 4), np.uint64)
            self._call("sdtree_read_dtree_nodes", C.c_int32(which), _fp(sums), _p(ch, C.c_uint16), _p(fx, C.c_uint64))
            out[name] = {"offset": off, "num_nodes": nn, "max_depth": md, "sum": sm, "stat_weight": sw,
                         "node_sums": sums, "node_children": ch, "node_fixed": fx}
        theta = np.zeros(n, np.float32)
        self._call("sdtree_read_adam", _fp(theta))
        out["theta"] = theta
        return out

    def query_pdf(self, positions, dirs):
        p = np.ascontiguousarray(positions, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        out = np.empty(p.shape[0], np.float32)
        self._call("query_pdf", C.c_uint32(p.shape[0]), _fp(p), _fp(d), _fp(out))
        return out

    def query_sample(self, positions, seed):
        p = np.ascontiguousarray(positions, np.float32)
        out = np.empty((p.shape[0], 3), np.float32)
        self._call("query_sample", C.c_uint32(p.shape[0]), _fp(p), C.c_uint64(seed), _fp(out))
        return out

    # -- HIP-only: device buffers and kernel timing --------------------------------------------
    def stat_buffers(self):
        ps, pw = C.c_void_p(), C.c_void_p()
        ns, nw = C.c_uint64(), C.c_uint64()
        self._call("sdtree_stat_buffers", C.byref(ps), C.byref(ns), C.byref(pw), C.byref(nw))
        return (ps.value, ns.value), (pw.value, nw.value)

    def film_buffers(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._call("film_buffers", C.byref(a), C.byref(b))
        return a.value, b.value

    def image_buffers(self):
        a, b, w = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._call("image_buffers", C.byref(a), C.byref(b), C.byref(w))
        self._image_w = w.value
        return a.value, b.value

    def image_weight_buffer(self):
        self.image_buffers()
        return self._image_w

    def final_partials(self):
        """Between render_passes_nostat() and finish_passes() of a sharded FINAL iteration (include/ppg.h "Final iteration: groups of passes"):
        (pointer, float count) of the buffer to all-reduce — device memory for the HIP engine, host memory for the oracle —, (None, 0) when
        this call's passes were not rendered in whole groups by rank."""
        ptr, n = C.c_void_p(), C.c_uint64()
        self._call("final_partials", C.byref(ptr), C.byref(n))
        return ptr.value, n.value

    def final_partials_commit(self):
        self._call("final_partials_commit")

    def final_partials_expected(self, n_passes):
        """Float count of the buffer final_partials() hands over for a sharded final iteration of n_passes passes — a function of what every
        rank knows (film size, pass count), so that a rank that failed can still join the others' collective with zeros."""
        f = self._f("final_group_passes")
        f.restype, f.argtypes = C.c_int32, [C.c_int32]
        g = int(f(C.c_int32(int(n_passes))))
        n = self.width * self.height
        return 4 * n + (-(-int(n_passes) // g)) * 7 * n

    def adam_records(self):
        """Inside the round hook: (pointer, count) of this rank's 32-byte ppg_adam_record array (device memory for the HIP engine,
        host memory for the oracle)."""
        ptr, n = C.c_void_p(), C.c_uint64()
        self._call("adam_records", C.byref(ptr), C.byref(n))
        return ptr.value, n.value

    def adam_records_replace(self, ptr, n):
        """Inside the round hook: the records to apply instead (the union over all ranks)."""
        self._call("adam_records_replace", C.c_void_p(ptr), C.c_uint64(n))

    # ---- one owner per D-tree (include/ppg.h "Sharded optimiser") ----
    def hook_phase(self):
        """Inside the round hook: 0 before the round's records are applied, 1 after (only if phase 0 asked for the records by owner)."""
        ph = C.c_int32()
        self._call("hook_phase", C.byref(ph))
        return ph.value

    def adam_records_by_owner(self, world):
        """Phase 0: (pointer to this rank's records in key order, [count for owner 0, ..., owner world-1])."""
        ptr = C.c_void_p()
        counts = (C.c_uint64 * world)()
        self._call("adam_records_by_owner", C.c_int32(world), C.byref(ptr), counts)
        return ptr.value, [int(c) for c in counts]

    def adam_state(self, world):
        """Phase 1: (pointer to the packed optimiser state, 24 bytes per S-tree node, world * segment entries; segment)."""
        ptr, seg = C.c_void_p(), C.c_uint64()
        self._call("adam_state", C.c_int32(world), C.byref(ptr), C.byref(seg))
        return ptr.value, seg.value

    def adam_state_commit(self):
        self._call("adam_state_commit")

    def set_pass_hook(self, fn):
        """fn() is called at the end of every round of the sampling-fraction optimiser (include/ppg.h), after this rank's records
        were collected and before they are applied."""
        HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p)

        def tramp(_user):
            try:
                fn()
                return 0
            except Exception:  # pragma: no cover - surfaced as PPG_ERR_INVALID by the library
                import traceback
                traceback.print_exc()
                return 1
        self._hook_keep = HOOK(tramp) if fn is not None else HOOK(0)
        self._call("set_pass_hook", self._hook_keep, None)

    def set_footprint_hook(self, fn):
        """fn(dev_halo, n_floats, local_status): called whenever a sharded filtered film's footprint is complete (include/ppg.h "Footprint
        hook"); all-reduces the floats in place with the ranks' status words and raises if any rank failed.  dev_halo is None when the rank
        has no buffer to give (local_status != 0).  Install it BEFORE the filter and the shard meet; None clears it."""
        HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32)

        def tramp(_user, ptr, n, status):
            try:
                fn(ptr, int(n), int(status))
                return 0
            except Exception as ex:  # surfaced as PPG_ERR_INVALID by the library
                if type(ex).__name__ != "RenderAborted":  # (an abort the peers announced is the protocol at work, not a fault to report)
                    import traceback
                    traceback.print_exc()
                return 1
        keep = HOOK(tramp) if fn is not None else HOOK(0)
        self._call("set_footprint_hook", keep, None)
        self._foot_keep = keep  # (replaced only once the library has taken the new one: a refused clear leaves the old trampoline in use)

    def footprint_halo_floats(self, tile_size, world, border, width=None, height=None):
        """ppg_footprint_halo_floats for this engine's film (or width x height): 7 floats per border slot."""
        return footprint_halo_floats(self.width if width is None else width, self.height if height is None else height, tile_size, world, border, self.lib)

    def set_stop_hook(self, fn):
        """fn(local_stop) -> stop: asked after every batch of passes of a budgetType = seconds render (include/ppg.h ppg_set_stop_hook)."""
        HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)

        def tramp(_user, local):
            try:
                return int(fn(int(local)))
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1
        self._stop_keep = HOOK(tramp) if fn is not None else HOOK(0)
        self._call("set_stop_hook", self._stop_keep, None)

    def enable_kernel_timing(self, on=True):
        self._call("enable_kernel_timing", C.c_int32(int(on)))

    def kernel_times(self):
        arr = (KernelTime * 64)()
        n = C.c_uint32()
        self._call("kernel_times", arr, C.c_uint32(64), C.byref(n))
        return [dict(name=arr[i].name.decode(), ms=arr[i].ms, launches=arr[i].launches, units=arr[i].units)
                for i in range(n.value)]
