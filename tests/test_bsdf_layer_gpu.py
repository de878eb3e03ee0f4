"""Every compiled copy of the kernels' BSDF layer against the oracle, bit for bit, over LATTICE and EDGE of bsdf_cases.py, through
ppg_debug_bsdf_as (include/ppg_testhooks.h):

  FULL    mat_eval / mat_pdf / mat_sample of the TRACE unit of each kernel family 0 .. 5 (the families differ by preprocessor: PPG_MFD,
          PPG_COAT with the nested BSDF behind real calls, PPG_BLEND with the scene as a further argument)
  COMMON  the same functions inside the translation unit of k_shade<false, true, MSET_COMMON> (PPG_PARAM_TEXTURES = 0: another Mat, a
          computed mat_spec_lum)
  LEAN    bsdf_eval / bsdf_pdf / bsdf_sample of the base family, on a scene of diffuse / two-sided diffuse / mirror

One launch per copy with all materials concatenated; the oracle's records are test_bsdf_layer.py's, computed once."""
import numpy as np
import pytest

import bsdf_cases as bc
from conftest import CBOX_PROPS
from ppg_host.bindings import DEBUG_BSDF_ITEM_DTYPE
from test_bsdf_layer import oracle_all
from test_microfacet_general_gpu import hip, scene_with

f32 = np.float32
pytestmark = pytest.mark.gpu
FAMILIES = 6
COMMON_NAMES = [n for n, m in bc.MATERIALS if bc.in_common(m)]
COPIES = [("FULL-%d" % f, f, "FULL", bc.NAMES) for f in range(FAMILIES)] + [("COMMON", 0, "COMMON", COMMON_NAMES), ("LEAN", 0, "LEAN", bc.LEAN)]


def _items(names, base):
    """the items of `names`, concatenated, material base + k; -> (items, {name: slice})"""
    parts, where, at = [], {}, 0
    for k, name in enumerate(names):
        it = bc.items(name)
        a = np.zeros(len(it["wi"]), DEBUG_BSDF_ITEM_DTYPE)
        a["material"], a["wi"], a["wo"], a["sample"], a["key"] = base + k, it["wi"], it["wo"], it["u"], it["key"]
        parts.append(a)
        where[name] = slice(at, at + len(a))
        at += len(a)
    return np.concatenate(parts), where


@pytest.fixture(scope="module")
def runs():
    """{copy: (records, {name: slice})}: eight launches, and the old entry and family -1 over one material each"""
    out = {}
    desc, base = scene_with([m for _, m in bc.MATERIALS])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    items, where = _items(bc.NAMES, base)
    for copy, fam, unit, names in COPIES[:FAMILIES]:
        out[copy] = (e.debug_bsdf_as(items, family=fam, unit=unit), where)
    citems, cwhere = _items(COMMON_NAMES, 0)
    citems["material"] = items["material"][np.concatenate([np.arange(where[n].start, where[n].stop) for n in COMMON_NAMES])]
    out["COMMON"] = (e.debug_bsdf_as(citems, family=0, unit="COMMON"), cwhere)
    one = where["ggx-roughdielectric-0.3"]
    it = items[one]
    out["old entry"] = (e.debug_bsdf(it["material"], it["wi"], it["wo"], it["sample"], it["key"]), None)
    out["own"] = (e.debug_bsdf_as(it, family=-1, unit="LEAN"), None)  # (family -1 ignores the unit: the scene renders FULL)
    e.close()
    ldesc, lbase = scene_with([dict(bc.MATERIALS)[n] for n in bc.LEAN])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(ldesc)
    litems, lwhere = _items(bc.LEAN, lbase)
    out["LEAN"] = (e.debug_bsdf_as(litems, family=0, unit="LEAN"), lwhere)
    out["LEAN own"] = (e.debug_bsdf_as(litems[lwhere["twosided-diffuse"]], family=-1, unit="FULL"), None)  # (likewise: the scene renders LEAN)
    e.close()
    return out


def same(a, b):
    """bit for bit; a word that is a NaN on both sides counts as equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a == b
    a, b = a.astype(f32, copy=False), b.astype(f32, copy=False)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def can_succeed(mat, wi):
    """from this side the material can return a sample"""
    if mat.get("twosided") or mat.get("opacity") is not None or mat["type"] in ("dielectric", "thindielectric", "roughdielectric"):
        return np.ones(len(wi), bool)
    return wi[:, 2] > 0


@pytest.mark.parametrize("copy,fam,unit,names", COPIES, ids=[c[0] for c in COPIES])
def test_copy_equals_the_oracle_bit_for_bit(oracle_lib, runs, copy, fam, unit, names):
    rec, where = runs[copy]
    seen = set()
    for name in names:
        mat, it, o, g = dict(bc.MATERIALS)[name], bc.items(name), oracle_all(oracle_lib, name), rec[where[name]]
        for q, ref in (("eval", o["eval"]), ("pdf", o["epdf"]), ("weight", o["weight"])):
            ok = same(g[q], ref)
            assert ok.all(), (name, q, int((~ok).sum()), np.nonzero(~ok.reshape(len(g), -1).all(1))[0][:5])
        assert np.all(g["_pad"][:, 0] == o["flags"]) and not g["_pad"][:, 1].any(), (name, "flags")
        live = o["weight"].any(1)  # (a failed sample leaves the other fields of the record unspecified)
        for q, ref in (("wo", o["wo"]), ("sampled_pdf", o["pdf"]), ("eta", o["eta"]), ("delta", o["delta"]), ("is_null", o["null"])):
            ok = same(g[q][live], ref[live])
            assert ok.all(), (name, q, int((~ok).sum()), np.nonzero(live)[0][np.nonzero(~ok.reshape(live.sum(), -1).all(1))[0][:5]])
        # against silent passes: a quarter of the samples succeed where the material can succeed from that side
        lat = ~it["is_edge"] & can_succeed(mat, it["wi"])
        assert live[lat].mean() >= 0.25, (name, float(live[lat].mean()))
        e = it["is_edge"]
        seen |= {"wi:" + c for c in np.unique(it["wi_class"][e])} | {"wo:" + c for c in np.unique(it["wo_class"][e])}
        seen |= {"u:" + c for c in np.unique(it["u_class"][e & live])}
    missing = set(bc.EDGE_CLASSES) - seen
    assert not missing, missing  # every EDGE class contributes compared items to this copy


def _bytes(rec):
    return rec.view(np.uint8).reshape(len(rec), -1)


@pytest.mark.parametrize("name", bc.NAMES)
def test_the_six_full_copies_agree(runs, name):
    """identical bytes over the whole record, failed samples included"""
    first, where = runs["FULL-0"]
    for f in range(1, FAMILIES):
        assert np.array_equal(_bytes(first[where[name]]), _bytes(runs["FULL-%d" % f][0][where[name]])), f


@pytest.mark.parametrize("name", COMMON_NAMES)
def test_common_unit_equals_the_base_family(runs, name):
    """... plastic and roughplastic with a coloured specular among them: mat_spec_lum is computed in one unit and read in the other"""
    full, where = runs["FULL-0"]
    common, cwhere = runs["COMMON"]
    assert np.array_equal(_bytes(full[where[name]]), _bytes(common[cwhere[name]]))


def test_common_classes_hold_a_coloured_specular():
    col = [n for n in COMMON_NAMES if dict(bc.MATERIALS)[n]["type"] in ("plastic", "roughplastic") and len(set(dict(bc.MATERIALS)[n]["specular"])) == 3]
    assert {dict(bc.MATERIALS)[n]["type"] for n in col} == {"plastic", "roughplastic"}


@pytest.mark.parametrize("name", bc.LEAN)
def test_lean_functions_equal_the_base_family(runs, name):
    full, where = runs["FULL-0"]
    lean, lwhere = runs["LEAN"]
    assert np.array_equal(_bytes(full[where[name]]), _bytes(lean[lwhere[name]]))


def test_old_entry_and_family_minus_one(runs):
    """ppg_debug_bsdf is ppg_debug_bsdf_as(max(scene family, ext), FULL); family -1 is the scene's own family and FULL / LEAN setting"""
    where = runs["FULL-2"][1]["ggx-roughdielectric-0.3"]
    assert np.array_equal(_bytes(runs["old entry"][0]), _bytes(runs["FULL-2"][0][where]))
    assert np.array_equal(_bytes(runs["own"][0]), _bytes(runs["FULL-0"][0][where]))
    assert np.array_equal(_bytes(runs["LEAN own"][0]), _bytes(runs["LEAN"][0][runs["LEAN"][1]["twosided-diffuse"]]))


def _one(material, u=(0.5, 0.5)):
    a = np.zeros(1, DEBUG_BSDF_ITEM_DTYPE)
    a["material"], a["wi"], a["wo"], a["sample"] = material, (0, 0, 1), (0, 0, 1), u
    return a


def test_refusals():
    """the contract of include/ppg_testhooks.h: each refusal names its reason and launches nothing"""
    import ppg_host
    PPGError = ppg_host.PPGError
    mats = [dict(bc.MATERIALS)[n] for n in ("plastic", "dielectric-1.5", "mask-diffuse")] + [dict(dict(bc.MATERIALS)["plastic"], specular_texture=0)]
    desc, base = scene_with(mats)
    desc.textures = [dict(rgb=np.full((2, 2, 3), 0.5, f32))]
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    n_mat = len(desc.materials)

    def refused(match, code=-1, **kw):
        with pytest.raises(PPGError, match=match) as ei:
            e.debug_bsdf_as(kw.pop("items", _one(base)), **kw)
        assert ei.value.code == code

    refused("kernel family", family=FAMILIES)
    refused("kernel family", family=-2)
    refused("no such unit", family=0, unit=3)
    refused("base family", family=2, unit="LEAN")
    refused("base family", family=1, unit="COMMON")
    refused("FULL", family=0, unit="LEAN")
    refused("common classes", family=0, unit="COMMON", items=_one(base + 1))
    refused("masked", family=0, unit="COMMON", items=_one(base + 2))
    refused("bitmap", family=0, unit="COMMON", items=_one(base + 3))
    refused("out of range", family=0, items=_one(n_mat))
    refused("out of range", family=0, items=_one(-1))
    for bad in ((1.0000001, 0.5), (0.5, 1.5), (-1e-9, 0.5), (0.5, np.nan), (np.inf, 0.5)):
        refused("outside", family=0, items=_one(base, bad))
        with pytest.raises(PPGError, match="outside"):
            e.debug_bsdf(base, (0, 0, 1), (0, 0, 1), bad)
    assert len(e.debug_bsdf_as(_one(base)[:0], family=0)) == 0
    assert e.debug_bsdf_as(_one(base), family=0, unit="COMMON")["weight"].any()
    e.begin_render()
    refused("ppg_begin_render", code=-3, family=0)
    e.end_render()
    e.close()


def test_a_family_below_the_scenes_own_is_refused_and_the_horizon_is_sampled():
    """A scene with a general microfacet entry needs the ext family.  Its roughconductor with all normals sampled shows what the oracle
    cannot (test_bsdf_layer.py): roughconductor.cpp:370 refuses wi.z < 0, so wi.z = +0 and -0 are sampled, and a normal that sends wo above
    the horizon gives a sample (microfacet.h:356-358: the density of all normals does not look at wi)."""
    import ppg_host
    desc, base = scene_with([dict(bc.GOLD, alpha=0.3, sample_visible=False), dict(bc.GOLD, alpha=0.3, sample_visible=False, distribution="beckmann")])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    for fam in (0, 1):
        with pytest.raises(ppg_host.PPGError, match="kernel family") as ei:
            e.debug_bsdf_as(_one(base), family=fam)
        assert ei.value.code == -1
    it = bc.items("ggx-0.25")
    hor = np.nonzero(it["wi"][:, 2] == 0)[0]
    a = np.zeros(2 * len(hor), DEBUG_BSDF_ITEM_DTYPE)
    a["material"] = np.repeat([base, base + 1], len(hor))
    for q, src in (("wi", "wi"), ("wo", "wo"), ("sample", "u")):
        a[q] = np.tile(it[src][hor], (2, 1))
    recs = [e.debug_bsdf_as(a, family=fam) for fam in (-1, 5)]
    e.close()
    assert np.array_equal(_bytes(recs[0]), _bytes(recs[1]))
    r = recs[0]
    live = r["weight"].any(1)
    for m in (0, 1):
        for neg in (False, True):
            sel = (a["material"] == base + m) & (np.signbit(a["wi"][:, 2]) == neg)
            assert sel.sum() == 144 and live[sel].sum() >= 20, (m, neg, int(live[sel].sum()))
    # (the weight itself is D G (wi . m) / (pdf cosTheta(wi)) with G = 0 and cosTheta(wi) = 0, roughconductor.cpp:399-401 and microfacet.h:
    # 479-480: 0 / 0 in the reference too, so its value is asserted nowhere; a NaN counts as "not black" above)
    assert np.all(r["wo"][live, 2] > 0) and np.all(r["sampled_pdf"][live] > 0)
