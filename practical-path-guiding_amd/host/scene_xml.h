/*
 * scene_xml.h — C++ loader for the subset of Mitsuba 0.6 scene XML the reference's bundled scenes use, so that
 * `ppg_render scene.xml` reads what `mitsuba scene.xml` reads:
 *
 *   integrator  guided_path (properties of guided_path.cpp:1014-1085 and integrator.cpp:192-218)
 *   sensor      perspective (fov, fovAxis, nearClip, farClip, toWorld), film hdrfilm (width, height; rfilter box)
 *   shapes      sphere (center, radius, toWorld = rotation x uniform scale, flipNormals; analytic), disk (toWorld, flipNormals; analytic), cylinder (p0, p1, radius, toWorld, flipNormals; analytic), obj (filename, toWorld, faceNormals, flipNormals, flipTexCoords, collapse), rectangle (toWorld, flipNormals)
 *   bsdfs       diffuse, conductor, roughconductor / roughdielectric / roughplastic (ggx / beckmann, isotropic; roughplastic reads Mitsuba's data/microfacet tables), plastic, dielectric, thindielectric, mask (constant opacity),
 *               twosided(BRDF) — top level with id, nested, or <ref id>
 *   emitters    point, spot, directional (SceneData::deltaEmitters; ppg_set_delta_emitters), area (nested in a shape), constant (environment), envmap (latitude-longitude .exr / .pfm / .hdr; filename, scale, toWorld = rotation),
 *               sunsky (baked into an envmap at load time, host/sunsky.h; its tables are parsed from the operator's Mitsuba source tree)
 *   values      <spectrum>, <rgb>, <srgb>; <transform> of translate / rotate / scale / lookAt / matrix; <default> and $name
 *
 * Anything else throws std::runtime_error naming the plugin.  Same semantics as ppg_host/mitsuba_xml.py (the two are tested against each
 * other); the OBJ reader follows shapes/obj.cpp:198-342 and TriMesh::computeNormals (trimesh.cpp:608-676).  Header only.
 */
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "guided_path_hip.h"
#include "rough_transmittance.h"
#include "hdr_image.h"

namespace ppg {

// ------------------------------------------------------------------------------------------------ minimal XML
struct XmlNode {
    std::string tag;
    std::vector<std::pair<std::string, std::string>> attrs;
    std::vector<XmlNode> children;
    const std::string *attr(const std::string &k) const {
        for (auto &a : attrs) if (a.first == k) return &a.second;
        return nullptr;
    }
    std::string get(const std::string &k, const std::string &d = "") const { auto *a = attr(k); return a ? *a : d; }
    const XmlNode *child(const std::string &t) const {
        for (auto &c : children) if (c.tag == t) return &c;
        return nullptr;
    }
};

class XmlParser {
public:
    explicit XmlParser(const std::string &text) : s(text), p(0) {}
    XmlNode parseDocument() {
        skipMisc();
        XmlNode root = parseElement();
        return root;
    }

private:
    const std::string &s;
    size_t p;
    [[noreturn]] void fail(const std::string &m) const { throw std::runtime_error("XML: " + m + " at offset " + std::to_string(p)); }
    void skipWs() { while (p < s.size() && std::isspace((unsigned char)s[p])) ++p; }
    bool starts(const char *t) const { return s.compare(p, strlen(t), t) == 0; }
    void skipMisc() {
        for (;;) {
            skipWs();
            if (starts("<?")) { size_t e = s.find("?>", p); if (e == std::string::npos) fail("unterminated <?"); p = e + 2; }
            else if (starts("<!--")) { size_t e = s.find("-->", p); if (e == std::string::npos) fail("unterminated comment"); p = e + 3; }
            else if (starts("<!")) { size_t e = s.find('>', p); if (e == std::string::npos) fail("unterminated <!"); p = e + 1; }
            else break;
        }
    }
    static std::string unescape(const std::string &v) {
        std::string o;
        for (size_t i = 0; i < v.size(); ++i) {
            if (v[i] != '&') { o += v[i]; continue; }
            static const std::pair<const char *, char> ent[] = {{"&quot;", '"'}, {"&amp;", '&'}, {"&lt;", '<'}, {"&gt;", '>'}, {"&apos;", '\''}};
            bool done = false;
            for (auto &e : ent) if (v.compare(i, strlen(e.first), e.first) == 0) { o += e.second; i += strlen(e.first) - 1; done = true; break; }
            if (!done) o += v[i];
        }
        return o;
    }
    std::string name() {
        size_t b = p;
        while (p < s.size() && (std::isalnum((unsigned char)s[p]) || s[p] == '_' || s[p] == '-' || s[p] == ':' || s[p] == '.')) ++p;
        if (p == b) fail("name expected");
        return s.substr(b, p - b);
    }
    XmlNode parseElement() {
        if (p >= s.size() || s[p] != '<') fail("'<' expected");
        ++p;
        XmlNode n;
        n.tag = name();
        for (;;) {
            skipWs();
            if (p >= s.size()) fail("unterminated tag");
            if (s[p] == '/') { if (s.compare(p, 2, "/>") != 0) fail("'/>' expected"); p += 2; return n; }
            if (s[p] == '>') { ++p; break; }
            std::string k = name();
            skipWs();
            if (p >= s.size() || s[p] != '=') fail("'=' expected");
            ++p; skipWs();
            if (p >= s.size() || (s[p] != '"' && s[p] != '\'')) fail("quoted value expected");
            char q = s[p++];
            size_t e = s.find(q, p);
            if (e == std::string::npos) fail("unterminated attribute");
            n.attrs.emplace_back(k, unescape(s.substr(p, e - p)));
            p = e + 1;
        }
        for (;;) {  // content
            size_t lt = s.find('<', p);
            if (lt == std::string::npos) fail("unterminated element <" + n.tag + ">");
            p = lt;
            if (starts("<!--")) { size_t e = s.find("-->", p); if (e == std::string::npos) fail("unterminated comment"); p = e + 3; continue; }
            if (starts("</")) {
                p += 2;
                std::string t = name();
                if (t != n.tag) fail("</" + t + "> closes <" + n.tag + ">");
                skipWs();
                if (p >= s.size() || s[p] != '>') fail("'>' expected");
                ++p;
                return n;
            }
            n.children.push_back(parseElement());
        }
    }
};

// ------------------------------------------------------------------------------------------------ small float algebra
struct Mat4 {
    float m[16];
    static Mat4 identity() { Mat4 r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1; return r; }
    Mat4 operator*(const Mat4 &o) const {
        Mat4 r{};
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { float a = 0; for (int k = 0; k < 4; ++k) a += m[4 * i + k] * o.m[4 * k + j]; r.m[4 * i + j] = a; }
        return r;
    }
};
struct V3 { float x, y, z; };
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 normalized(V3 a) { float l = std::sqrt(dot(a, a)); return {a.x / l, a.y / l, a.z / l}; }
inline V3 xfPoint(const Mat4 &m, V3 p) {
    float x = m.m[0] * p.x + m.m[1] * p.y + m.m[2] * p.z + m.m[3], y = m.m[4] * p.x + m.m[5] * p.y + m.m[6] * p.z + m.m[7];
    float z = m.m[8] * p.x + m.m[9] * p.y + m.m[10] * p.z + m.m[11], w = m.m[12] * p.x + m.m[13] * p.y + m.m[14] * p.z + m.m[15];
    if (w != 1) { x /= w; y /= w; z /= w; }
    return {x, y, z};
}
// inverse transpose of the upper 3x3 in double (Transform::operator()(Normal))
inline void normalMatrix(const Mat4 &m, double out[9]) {
    const double a = m.m[0], b = m.m[1], c = m.m[2], d = m.m[4], e = m.m[5], f = m.m[6], g = m.m[8], h = m.m[9], i = m.m[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det, (f * g - d * i) / det, (a * i - c * g) / det,
                           (c * d - a * f) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
    for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) out[3 * r + cc] = inv[3 * cc + r];  // transpose
}
inline V3 xfNormal(const double nm[9], V3 n) {
    return {(float)(nm[0] * n.x + nm[1] * n.y + nm[2] * n.z), (float)(nm[3] * n.x + nm[4] * n.y + nm[5] * n.z), (float)(nm[6] * n.x + nm[7] * n.y + nm[8] * n.z)};
}

// ------------------------------------------------------------------------------------------------ colour values (ppg_host/spectrum.py)
namespace detail {
static const double kCIE[471][3] = {
#include "cie1931_xyz_1nm.inc"
};
inline double evalInterp(const std::vector<double> &lam, const std::vector<double> &val, double g) {  // incl. the reversed lerp, spectrum.cpp:693-706
    if (lam.size() < 2 || g < lam.front() || g > lam.back()) return 0.0;
    size_t i = std::lower_bound(lam.begin(), lam.end(), g) - lam.begin();
    if (lam[std::min(i, lam.size() - 1)] == g) return val[std::min(i, lam.size() - 1)];
    i = std::max<size_t>(1, std::min(i, lam.size() - 1));
    const double a = lam[i - 1], b = lam[i], fa = val[i - 1], fb = val[i], t = (g - a) / (b - a);
    return (1 - t) * fb + t * fa;
}
}  // namespace detail

// scene-file spectra are zero-extended and clamped (scenehandler.cpp:563-566); the conductor plug-ins read data/ior/*.spd without either
inline void interpolatedToRGB(std::vector<double> lam, std::vector<double> val, float rgb[3], bool zeroExtend = true, bool clamp = true) {
    using namespace detail;
    const double spacing = (lam.back() - lam.front()) / (lam.size() - 1);  // zeroExtend, spectrum.cpp:630-648
    if (zeroExtend && val.front() != 0) { lam.insert(lam.begin(), lam.front() - spacing); val.insert(val.begin(), 0.0); }
    if (zeroExtend && val.back() != 0) { lam.push_back(lam.back() + spacing); val.push_back(0.0); }
    std::vector<double> wl(471), cx(471), cy(471), cz(471);
    for (int i = 0; i < 471; ++i) { wl[i] = 360.0 + i; cx[i] = kCIE[i][0]; cy[i] = kCIE[i][1]; cz[i] = kCIE[i][2]; }
    const double step = 0.00731;  // off-node sampling: exact hits have measure zero
    double X = 0, Y = 0, Z = 0, N = 0, pg = 0, ps[4] = {0, 0, 0, 0};
    bool first = true;
    for (long k = 0;; ++k) {
        const double g = 360.0 + k * step;
        if (!(g < 830.0)) break;
        const double s = evalInterp(lam, val, g), x = evalInterp(wl, cx, g), y = evalInterp(wl, cy, g), z = evalInterp(wl, cz, g);
        const double cur[4] = {s * x, s * y, s * z, y};
        if (!first) { const double h = 0.5 * (g - pg); X += h * (cur[0] + ps[0]); Y += h * (cur[1] + ps[1]); Z += h * (cur[2] + ps[2]); N += h * (cur[3] + ps[3]); }
        first = false; pg = g;
        for (int c = 0; c < 4; ++c) ps[c] = cur[c];
    }
    X /= N; Y /= N; Z /= N;
    const double r = 3.240479 * X - 1.537150 * Y - 0.498535 * Z, gg = -0.969256 * X + 1.875991 * Y + 0.041556 * Z, b = 0.055648 * X - 0.204043 * Y + 1.057311 * Z;
    rgb[0] = (float)(clamp ? std::max(r, 0.0) : r); rgb[1] = (float)(clamp ? std::max(gg, 0.0) : gg); rgb[2] = (float)(clamp ? std::max(b, 0.0) : b);
}

// InterpolatedSpectrum(path), spectrum.cpp:575-600: "wavelength value" lines, # comments; stops at the first malformed line
inline bool readSPD(const std::string &path, std::vector<double> &lam, std::vector<double> &val) {
    std::ifstream sf(path);
    if (!sf) return false;
    std::string line;
    while (std::getline(sf, line)) {
        const size_t a = line.find_first_not_of(" \t\r\n");
        if (a == std::string::npos || line[a] == '#') continue;
        std::istringstream ls(line);
        double l, v;
        if (!(ls >> l >> v)) break;
        lam.push_back(l); val.push_back(v);
    }
    return true;
}

// <blackbody temperature=".." scale=".."/> (scenehandler.cpp:534-547): Planck's law (BlackBodySpectrum::eval, spectrum.cpp:483-495) through
// Spectrum::fromContinuousSpectrum, clamped, times scale
inline void blackbodyToRGB(double temperature, double scale, float rgb[3]) {
    using namespace detail;
    std::vector<double> wl(471), cx(471), cy(471), cz(471);
    for (int i = 0; i < 471; ++i) { wl[i] = 360.0 + i; cx[i] = kCIE[i][0]; cy[i] = kCIE[i][1]; cz[i] = kCIE[i][2]; }
    const double step = 0.00731, cc = 299792458.0, k = 1.3806488e-23, h = 6.62606957e-34;
    double X = 0, Y = 0, Z = 0, N = 0, pg = 0, ps[4] = {0, 0, 0, 0};
    bool first = true;
    for (long n = 0;; ++n) {
        const double g = 360.0 + n * step;
        if (!(g < 830.0)) break;
        const double lambda = g * 1e-9;
        const double s = (2 * h * cc * cc) * std::pow(lambda, -5.0) / ((std::exp((h / k) * cc / (lambda * temperature)) - 1.0) * 1e9);
        const double x = evalInterp(wl, cx, g), y = evalInterp(wl, cy, g), z = evalInterp(wl, cz, g);
        const double cur[4] = {s * x, s * y, s * z, y};
        if (!first) { const double hh = 0.5 * (g - pg); X += hh * (cur[0] + ps[0]); Y += hh * (cur[1] + ps[1]); Z += hh * (cur[2] + ps[2]); N += hh * (cur[3] + ps[3]); }
        first = false; pg = g;
        for (int c = 0; c < 4; ++c) ps[c] = cur[c];
    }
    X /= N; Y /= N; Z /= N;
    const double r = 3.240479 * X - 1.537150 * Y - 0.498535 * Z, gg = -0.969256 * X + 1.875991 * Y + 0.041556 * Z, b = 0.055648 * X - 0.204043 * Y + 1.057311 * Z;
    rgb[0] = (float)std::max(r, 0.0) * (float)scale; rgb[1] = (float)std::max(gg, 0.0) * (float)scale; rgb[2] = (float)std::max(b, 0.0) * (float)scale;
}

}  // namespace ppg
#include "sunsky.h"
namespace ppg {

inline std::vector<double> parseFloats(std::string t) {
    for (char &c : t) if (c == ',') c = ' ';
    std::istringstream is(t);
    std::vector<double> v;
    double x;
    while (is >> x) v.push_back(x);
    return v;
}

inline void parseColour(const std::string &tag, const std::string &value, float rgb[3]) {
    if (tag == "rgb" || tag == "srgb") {
        double c[3];
        std::string v = value;
        v.erase(0, v.find_first_not_of(" \t"));
        if (!v.empty() && v[0] == '#') {
            for (int k = 0; k < 3; ++k) c[k] = std::stoi(v.substr(1 + 2 * k, 2), nullptr, 16) / 255.0;
        } else {
            auto f = parseFloats(v);
            if (f.size() == 1) f = {f[0], f[0], f[0]};
            if (f.size() != 3) throw std::runtime_error("expected 1 or 3 colour components, got '" + value + "'");
            for (int k = 0; k < 3; ++k) c[k] = f[k];
        }
        for (int k = 0; k < 3; ++k) rgb[k] = (float)(tag == "srgb" ? (c[k] <= 0.04045 ? c[k] / 12.92 : std::pow((c[k] + 0.055) / 1.055, 2.4)) : c[k]);
        return;
    }
    if (tag == "spectrum") {
        if (value.find(':') != std::string::npos) {
            std::string t = value;
            for (char &ch : t) if (ch == ',' || ch == ':') ch = ' ';
            auto f = parseFloats(t);
            std::vector<double> lam, val;
            for (size_t k = 0; k + 1 < f.size(); k += 2) { lam.push_back(f[k]); val.push_back(f[k + 1]); }
            interpolatedToRGB(lam, val, rgb);
            return;
        }
        auto f = parseFloats(value);
        if (f.size() == 1) { rgb[0] = rgb[1] = rgb[2] = (float)f[0]; return; }
        if (f.size() == 3) { for (int k = 0; k < 3; ++k) rgb[k] = (float)f[k]; return; }
    }
    throw std::runtime_error("unsupported colour element <" + tag + " value=\"" + value + "\">");
}

// ------------------------------------------------------------------------------------------------ OBJ (shapes/obj.cpp:198-342)
struct Mesh {
    std::vector<V3> positions, normals;  // normals empty = none
    std::vector<uint32_t> indices;
    std::vector<std::pair<float, float>> uvs;  // per-vertex texture coordinates, empty = none (kept for obj meshes only, as in ppg_host/mitsuba_xml.py)
};

inline float unitAngle(V3 u, V3 v) {  // util.h:309-314
    V3 s{v.x + u.x, v.y + u.y, v.z + u.z}, d{v.x - u.x, v.y - u.y, v.z - u.z};
    if (dot(u, v) < 0) return 3.14159265358979323846f - 2 * std::asin(0.5f * std::sqrt(dot(s, s)));
    return 2 * std::asin(0.5f * std::sqrt(dot(d, d)));
}

inline void computeNormals(Mesh &m, bool flip) {  // TriMesh::computeNormals, smooth branch (trimesh.cpp:631-671)
    m.normals.assign(m.positions.size(), V3{0, 0, 0});
    for (size_t t = 0; t + 2 < m.indices.size(); t += 3) {
        V3 n{0, 0, 0};
        for (int i = 0; i < 3; ++i) {
            const V3 &v0 = m.positions[m.indices[t + i]], &v1 = m.positions[m.indices[t + (i + 1) % 3]], &v2 = m.positions[m.indices[t + (i + 2) % 3]];
            V3 sideA = v1 - v0, sideB = v2 - v0;
            if (i == 0) {
                n = cross(sideA, sideB);
                float len = std::sqrt(dot(n, n));
                if (len == 0) break;
                n = {n.x / len, n.y / len, n.z / len};
            }
            float angle = unitAngle(normalized(sideA), normalized(sideB));
            V3 &dst = m.normals[m.indices[t + i]];
            dst = {dst.x + n.x * angle, dst.y + n.y * angle, dst.z + n.z * angle};
        }
    }
    for (V3 &n : m.normals) {
        float len = std::sqrt(dot(n, n));
        if (flip) len *= -1;
        if (len != 0) n = {n.x / len, n.y / len, n.z / len};
        else n = {1, 0, 0};
    }
}

/* TriMesh::rebuildTopology (trimesh.cpp:468-608): vertices re-merged on (position[, uv]); around each, the incident triangles are
 * clustered greedily by face normal (one new vertex per cluster of faces within maxAngle degrees of the cluster's first face), so that
 * the smooth normals computed afterwards stop at creases.  New vertices are numbered in the reference's order. */
inline void rebuildTopology(Mesh &m, std::vector<std::pair<float, float>> *uvs, float maxAngle) {
    const float dpThresh = std::cos(maxAngle * (float)(M_PI / 180.0));
    const size_t nt = m.indices.size() / 3;
    std::vector<V3> fn(nt);
    for (size_t t = 0; t < nt; ++t) {
        const V3 v0 = m.positions[m.indices[3 * t]], v1 = m.positions[m.indices[3 * t + 1]], v2 = m.positions[m.indices[3 * t + 2]];
        V3 n = cross(v1 - v0, v2 - v0);
        const float l = std::sqrt(dot(n, n));
        fn[t] = l > 2.93873587705571876e-39f ? V3{n.x / l, n.y / l, n.z / l} : V3{0, 0, 0};  // RCPOVERFLOW_FLT
    }
    struct Key { float v[5]; int n; bool operator<(const Key &o) const { return std::lexicographical_compare(v, v + n, o.v, o.v + o.n); } };
    std::multimap<Key, std::pair<uint32_t, bool>> vertexToFace;  // equal keys keep their insertion order (triangle, corner)
    for (size_t t = 0; t < nt; ++t)
        for (int j = 0; j < 3; ++j) {
            const uint32_t v = m.indices[3 * t + j];
            Key k{{m.positions[v].x, m.positions[v].y, m.positions[v].z, uvs ? (*uvs)[v].first : 0.0f, uvs ? (*uvs)[v].second : 0.0f}, uvs ? 5 : 3};
            vertexToFace.insert({k, {(uint32_t)t, false}});
        }
    std::vector<V3> newPositions;
    std::vector<std::pair<float, float>> newUVs;
    std::vector<uint32_t> newIndices(m.indices.size(), 0xFFFFFFFFu);
    for (auto it = vertexToFace.begin(); it != vertexToFace.end();) {
        auto end = vertexToFace.upper_bound(it->first);
        const V3 p{it->first.v[0], it->first.v[1], it->first.v[2]};
        for (auto it2 = it; it2 != end; ++it2) {
            if (it2->second.second) continue;
            const V3 n1 = fn[it2->second.first];
            const uint32_t vertexIdx = (uint32_t)newPositions.size();
            newPositions.push_back(p);
            if (uvs) newUVs.emplace_back(it->first.v[3], it->first.v[4]);
            for (auto it3 = it2; it3 != end; ++it3) {
                if (it3->second.second) continue;
                const V3 n2 = fn[it3->second.first];
                if ((n1.x == n2.x && n1.y == n2.y && n1.z == n2.z) || dot(n1, n2) > dpThresh) {
                    for (int i = 0; i < 3; ++i) {
                        const V3 q = m.positions[m.indices[3 * it3->second.first + i]];
                        if (q.x == p.x && q.y == p.y && q.z == p.z) newIndices[3 * it3->second.first + i] = vertexIdx;
                    }
                    it3->second.second = true;
                }
            }
        }
        it = end;
    }
    m.positions.swap(newPositions);
    m.indices.swap(newIndices);
    m.normals.clear();
    if (uvs) uvs->swap(newUVs);
}

inline std::vector<Mesh> loadOBJ(const std::string &path, const Mat4 &toWorld, bool faceNormals, bool flipNormals, bool flipTexCoords, bool collapse,
                                 float maxSmoothAngle = -1.0f) {
    std::ifstream is(path);
    if (!is) throw std::runtime_error("Wavefront OBJ file '" + path + "' not found!");
    std::vector<V3> V, N;
    std::vector<std::pair<float, float>> UV;
    struct Corner { int p, uv, n; };
    std::vector<Corner> tris;  // 3 per triangle
    std::vector<Mesh> meshes;
    double nm[9];
    normalMatrix(toWorld, nm);
    auto flush = [&]() {
        if (tris.empty()) return;
        std::vector<V3> pw(V.size()), nw(N.size());
        for (size_t i = 0; i < V.size(); ++i) pw[i] = xfPoint(toWorld, V[i]);
        for (size_t i = 0; i < N.size(); ++i) {
            V3 n = xfNormal(nm, N[i]);
            float l = std::sqrt(dot(n, n));
            nw[i] = l != 0 ? V3{n.x / l, n.y / l, n.z / l} : n;
        }
        struct Key { float v[8]; bool operator<(const Key &o) const { return std::lexicographical_compare(v, v + 8, o.v, o.v + 8); } };
        std::map<Key, uint32_t> vmap;
        Mesh m;
        std::vector<V3> vn;
        std::vector<std::pair<float, float>> vuv;
        bool hasNormals = false, hasUVs = false;
        for (const Corner &c : tris) {
            int p = c.p, n = c.n, uv = c.uv;
            if (p < 0) p += (int)V.size() + 1;
            if (n < 0) n += (int)N.size() + 1;
            if (uv < 0) uv += (int)UV.size() + 1;
            if (p <= 0 || p > (int)V.size()) throw std::runtime_error(path + ": vertex index out of bounds");
            if (n > (int)N.size() || uv > (int)UV.size()) throw std::runtime_error(path + ": normal / uv index out of bounds");
            V3 pn = n ? nw[n - 1] : V3{0, 0, 0};
            hasNormals |= n != 0;
            hasUVs |= uv != 0;
            std::pair<float, float> puv = uv ? UV[uv - 1] : std::make_pair(0.0f, 0.0f);
            Key k{{pw[p - 1].x, pw[p - 1].y, pw[p - 1].z, pn.x, pn.y, pn.z, puv.first, puv.second}};
            auto it = vmap.find(k);
            uint32_t id;
            if (it == vmap.end()) { id = (uint32_t)m.positions.size(); vmap[k] = id; m.positions.push_back(pw[p - 1]); vn.push_back(pn); vuv.push_back(puv); }
            else id = it->second;
            m.indices.push_back(id);
        }
        if (maxSmoothAngle >= 0) { rebuildTopology(m, hasUVs ? &vuv : nullptr, maxSmoothAngle); hasNormals = false; }  // obj.cpp:336-343
        if (faceNormals) {
            if (flipNormals) for (size_t t = 0; t + 2 < m.indices.size(); t += 3) std::swap(m.indices[t], m.indices[t + 1]);
        } else if (hasNormals) {
            m.normals = vn;
            if (flipNormals) for (V3 &n : m.normals) n = {-n.x, -n.y, -n.z};
        } else {
            computeNormals(m, flipNormals);
        }
        if (hasUVs) m.uvs = vuv;
        meshes.push_back(std::move(m));
        tris.clear();
    };
    std::string line, pending;
    auto handle = [&](const std::string &ln) {
        std::istringstream iss(ln);
        std::string buf;
        if (!(iss >> buf)) return;
        if (buf == "v") { V3 p{0, 0, 0}; iss >> p.x >> p.y >> p.z; V.push_back(p); }
        else if (buf == "vn") { V3 n{0, 0, 0}; iss >> n.x >> n.y >> n.z; N.push_back(n); }
        else if (buf == "vt") { float u = 0, v = 0; iss >> u >> v; UV.emplace_back(u, flipTexCoords ? 1 - v : v); }
        else if (buf == "g" && !collapse) flush();
        else if (buf == "usemtl") { if (!collapse) flush(); }
        else if (buf == "f") {
            std::vector<Corner> cs;
            std::string tok;
            while (iss >> tok) {
                Corner c{0, 0, 0};
                size_t a = tok.find('/');
                c.p = std::atoi(tok.substr(0, a).c_str());
                if (a != std::string::npos) {
                    size_t b = tok.find('/', a + 1);
                    std::string suv = tok.substr(a + 1, b == std::string::npos ? std::string::npos : b - a - 1);
                    if (!suv.empty()) c.uv = std::atoi(suv.c_str());
                    if (b != std::string::npos && b + 1 < tok.size()) c.n = std::atoi(tok.substr(b + 1).c_str());
                }
                cs.push_back(c);
            }
            if (cs.size() < 3) throw std::runtime_error(path + ": face with fewer than 3 vertices");
            for (size_t k = 1; k + 1 < cs.size(); ++k) { tris.push_back(cs[0]); tris.push_back(cs[k]); tris.push_back(cs[k + 1]); }  // fan
        }
    };
    while (std::getline(is, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n' || line.back() == '\t' || line.back() == ' ')) line.pop_back();
        if (!line.empty() && line.back() == '\\') { line.pop_back(); pending += line; continue; }  // obj.cpp:166-188
        handle(pending + line);
        pending.clear();
    }
    if (!pending.empty()) handle(pending);
    flush();
    return meshes;
}

/* shapes/serialized.cpp:148-212 + TriMesh::loadCompressed (trimesh.cpp:175-295): Mitsuba's binary mesh format — header 0x041C, version 3 or
 * 4, then a zlib stream {flags, [name], vertex count, triangle count, positions, [normals], [texcoords], [colours], indices}; several
 * meshes per file are addressed through the offset table at the end (shapeIndex). */
inline Mesh loadSerialized(const std::string &path, const Mat4 &toWorld, int shapeIndex, bool faceNormals, bool flipNormals, float maxSmoothAngle) {
    const std::vector<unsigned char> buf = slurp(path, "serialized");
    auto header = [&](size_t off) {
        uint16_t h[2];
        if (off + 4 > buf.size()) throw std::runtime_error(path + ": encountered an invalid file format!");
        memcpy(h, &buf[off], 4);
        if (h[0] != 0x041C) throw std::runtime_error(path + ": encountered an invalid file format!");
        if (h[1] != 3 && h[1] != 4) throw std::runtime_error(path + ": encountered an incompatible file version!");
        return (int)h[1];
    };
    const int version = header(0);
    size_t start = 0;
    if (shapeIndex != 0) {
        // the offset table at the end of the file (readOffset, trimesh.cpp:272-295); every size comes from the file: check it against the buffer
        // (the reference accepts shapeIndex == count and then reads past the table — an error here)
        if (buf.size() < 8) throw std::runtime_error(path + ": truncated file");
        uint32_t count;
        memcpy(&count, &buf[buf.size() - 4], 4);
        if (shapeIndex < 0 || (uint64_t)shapeIndex >= (uint64_t)count) throw std::runtime_error(path + ": shape index is out of range!");
        const uint64_t entry = version == 4 ? 8 : 4, back = entry * (uint64_t)(count - shapeIndex) + 4;
        if (back > buf.size()) throw std::runtime_error(path + ": corrupt offset table");
        if (version == 4) { uint64_t o; memcpy(&o, &buf[buf.size() - back], 8); if (o > buf.size()) throw std::runtime_error(path + ": corrupt offset table"); start = (size_t)o; }
        else { uint32_t o; memcpy(&o, &buf[buf.size() - back], 4); start = o; }
        if (start + 4 > buf.size()) throw std::runtime_error(path + ": corrupt offset table");
        header(start);
    }
    std::vector<unsigned char> data;
    {
        z_stream zs{};
        if (inflateInit(&zs) != Z_OK) throw std::runtime_error(path + ": zlib failure");
        zs.next_in = const_cast<unsigned char *>(&buf[start + 4]);
        zs.avail_in = (uInt)(buf.size() - start - 4);
        unsigned char chunk[1 << 16];
        int rc;
        do {
            zs.next_out = chunk; zs.avail_out = sizeof chunk;
            rc = inflate(&zs, Z_NO_FLUSH);
            if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&zs); throw std::runtime_error(path + ": corrupt zlib stream"); }
            data.insert(data.end(), chunk, chunk + (sizeof chunk - zs.avail_out));
        } while (rc != Z_STREAM_END);
        inflateEnd(&zs);
    }
    size_t off = 0;
    auto need = [&](size_t n) { if (off + n > data.size()) throw std::runtime_error(path + ": truncated mesh data"); };
    uint32_t flags;
    need(4); memcpy(&flags, &data[off], 4); off += 4;
    if (version == 4) { while (off < data.size() && data[off]) ++off; ++off; }
    uint64_t nv, nt;
    need(16); memcpy(&nv, &data[off], 8); memcpy(&nt, &data[off + 8], 8); off += 16;
    const bool dbl = (flags & 0x2000) != 0;
    if (nv > data.size() || nt > data.size()) throw std::runtime_error(path + ": truncated mesh data");  // every vertex / triangle takes > 1 byte: no overflow below
    auto take = [&](int comps, std::vector<float> &out) {
        const size_t n = (size_t)nv * comps;
        need(n * (dbl ? 8 : 4));
        out.resize(n);
        for (size_t k = 0; k < n; ++k) {
            if (dbl) { double v; memcpy(&v, &data[off + 8 * k], 8); out[k] = (float)v; }
            else memcpy(&out[k], &data[off + 4 * k], 4);
        }
        off += n * (dbl ? 8 : 4);
    };
    std::vector<float> P, N, UVs, C;
    take(3, P);
    if (flags & 0x0001) take(3, N);
    if (flags & 0x0002) take(2, UVs);
    if (flags & 0x0008) take(3, C);
    need((size_t)nt * 12);
    Mesh m;
    m.indices.resize((size_t)nt * 3);
    memcpy(m.indices.data(), &data[off], (size_t)nt * 12);
    for (uint32_t id : m.indices) if (id >= nv) throw std::runtime_error(path + ": vertex index out of bounds");
    bool identity = true;
    for (int k = 0; k < 16; ++k) identity &= toWorld.m[k] == Mat4::identity().m[k];
    double nm[9];
    normalMatrix(toWorld, nm);
    for (size_t i = 0; i < nv; ++i) {
        const V3 p{P[3 * i], P[3 * i + 1], P[3 * i + 2]};
        m.positions.push_back(identity ? p : xfPoint(toWorld, p));
        if (!N.empty()) {
            const V3 n{N[3 * i], N[3 * i + 1], N[3 * i + 2]};
            m.normals.push_back(identity ? n : normalized(xfNormal(nm, n)));
        }
    }
    const double a = toWorld.m[0], b = toWorld.m[1], c = toWorld.m[2], d = toWorld.m[4], e = toWorld.m[5], f = toWorld.m[6], g = toWorld.m[8], h = toWorld.m[9], i9 = toWorld.m[10];
    if (a * (e * i9 - f * h) - b * (d * i9 - f * g) + c * (d * h - e * g) < 0)
        for (size_t t = 0; t + 2 < m.indices.size(); t += 3) std::swap(m.indices[t], m.indices[t + 1]);
    std::vector<std::pair<float, float>> vuv;
    for (size_t i = 0; i + 1 < UVs.size(); i += 2) vuv.emplace_back(UVs[i], UVs[i + 1]);
    if (maxSmoothAngle >= 0) rebuildTopology(m, UVs.empty() ? nullptr : &vuv, maxSmoothAngle);
    if (faceNormals) {
        m.normals.clear();
        if (flipNormals) for (size_t t = 0; t + 2 < m.indices.size(); t += 3) std::swap(m.indices[t], m.indices[t + 1]);
    } else if (!m.normals.empty()) {
        if (flipNormals) for (V3 &n : m.normals) n = {-n.x, -n.y, -n.z};
    } else {
        computeNormals(m, flipNormals);
    }
    return m;
}

/* shapes/ply.cpp: Stanford PLY (ascii / binary little / big endian), vertex x y z [nx ny nz], faces of 3 or 4 indices (a quad becomes
 * (0, 1, 2), (3, 0, 2), ply.cpp:299-311); positions and normals go through toWorld as they are read (:229-233). */
inline Mesh loadPLY(const std::string &path, const Mat4 &toWorld, bool faceNormals, bool flipNormals, float maxSmoothAngle) {
    const std::vector<unsigned char> buf = slurp(path, "ply");
    const std::string all(buf.begin(), buf.end());
    const size_t end = all.find("end_header");
    if (all.compare(0, 3, "ply") != 0 || end == std::string::npos) throw std::runtime_error(path + ": not a PLY file");
    size_t off = all.find('\n', end) + 1;
    struct Prop { std::string name; bool list; std::string t0, t1; };
    struct Elem { std::string name; size_t count; std::vector<Prop> props; };
    std::vector<Elem> elems;
    std::string fmt;
    {
        std::istringstream hs(all.substr(0, end));
        std::string line;
        std::getline(hs, line);
        while (std::getline(hs, line)) {
            std::istringstream ls(line);
            std::string tok;
            if (!(ls >> tok) || tok == "comment" || tok == "obj_info") continue;
            if (tok == "format") ls >> fmt;
            else if (tok == "element") { Elem e; ls >> e.name >> e.count; elems.push_back(e); }
            else if (tok == "property" && !elems.empty()) {
                Prop p; std::string a;
                ls >> a;
                if (a == "list") { p.list = true; ls >> p.t0 >> p.t1 >> p.name; }
                else { p.list = false; p.t0 = a; ls >> p.name; }
                elems.back().props.push_back(p);
            }
        }
    }
    if (fmt != "ascii" && fmt != "binary_little_endian" && fmt != "binary_big_endian") throw std::runtime_error(path + ": unknown PLY format '" + fmt + "'");
    auto sizeOf = [&](const std::string &t) -> int {
        if (t == "char" || t == "int8" || t == "uchar" || t == "uint8") return 1;
        if (t == "short" || t == "int16" || t == "ushort" || t == "uint16") return 2;
        if (t == "int" || t == "int32" || t == "uint" || t == "uint32" || t == "float" || t == "float32") return 4;
        if (t == "double" || t == "float64") return 8;
        throw std::runtime_error(path + ": unknown PLY type '" + t + "'");
    };
    std::istringstream ascii(fmt == "ascii" ? all.substr(off) : std::string());
    const bool big = fmt == "binary_big_endian";
    auto next = [&](const std::string &t) -> double {
        if (fmt == "ascii") { double v; if (!(ascii >> v)) throw std::runtime_error(path + ": truncated PLY data"); return v; }
        const int n = sizeOf(t);
        if (off + n > buf.size()) throw std::runtime_error(path + ": truncated PLY data");
        unsigned char b[8];
        for (int k = 0; k < n; ++k) b[k] = buf[off + (big ? n - 1 - k : k)];
        off += n;
        if (t == "float" || t == "float32") { float v; memcpy(&v, b, 4); return v; }
        if (t == "double" || t == "float64") { double v; memcpy(&v, b, 8); return v; }
        if (t == "char" || t == "int8") return (signed char)b[0];
        if (t == "uchar" || t == "uint8") return b[0];
        if (t == "short" || t == "int16") { int16_t v; memcpy(&v, b, 2); return v; }
        if (t == "ushort" || t == "uint16") { uint16_t v; memcpy(&v, b, 2); return v; }
        if (t == "int" || t == "int32") { int32_t v; memcpy(&v, b, 4); return v; }
        uint32_t v; memcpy(&v, b, 4); return v;
    };
    std::map<std::string, std::vector<float>> cols;
    Mesh m;
    size_t nVerts = 0;
    for (const Elem &e : elems)
        for (size_t r = 0; r < e.count; ++r)
            for (const Prop &p : e.props) {
                if (p.list) {
                    const int n = (int)next(p.t0);
                    uint32_t v[4] = {0, 0, 0, 0};
                    const bool faceList = e.name == "face" && (p.name == "vertex_indices" || p.name == "vertex_index");
                    if (faceList && n != 3 && n != 4) throw std::runtime_error(path + ": only triangle and quad-based PLY meshes are supported");
                    for (int k = 0; k < n; ++k) { const double d = next(p.t1); if (k < 4) v[k] = (uint32_t)d; }
                    if (faceList) {
                        for (uint32_t id : {v[0], v[1], v[2]}) m.indices.push_back(id);
                        if (n == 4) for (uint32_t id : {v[3], v[0], v[2]}) m.indices.push_back(id);
                    }
                } else {
                    const double d = next(p.t0);
                    if (e.name == "vertex") { cols[p.name].push_back((float)d); if (p.name == "x") ++nVerts; }
                }
            }
    if (m.indices.empty() || nVerts == 0) throw std::runtime_error("Unable to load \"" + path + "\" (no triangles or vertices found)!");
    for (uint32_t id : m.indices) if (id >= nVerts) throw std::runtime_error(path + ": vertex index out of bounds");
    const bool hasN = cols.count("nx") && cols.count("ny") && cols.count("nz");
    double nm[9];
    normalMatrix(toWorld, nm);
    for (size_t i = 0; i < nVerts; ++i) {
        m.positions.push_back(xfPoint(toWorld, V3{cols["x"][i], cols["y"][i], cols["z"][i]}));
        if (hasN) m.normals.push_back(normalized(xfNormal(nm, V3{cols["nx"][i], cols["ny"][i], cols["nz"][i]})));
    }
    std::vector<std::pair<float, float>> vuv;
    const char *uvNames[2][2] = {{"u", "v"}, {"s", "t"}};
    for (auto &nmz : uvNames)
        if (cols.count(nmz[0]) && cols.count(nmz[1])) { vuv.clear(); for (size_t i = 0; i < nVerts; ++i) vuv.emplace_back(cols[nmz[0]][i], cols[nmz[1]][i]); }
    if (maxSmoothAngle >= 0) rebuildTopology(m, vuv.empty() ? nullptr : &vuv, maxSmoothAngle);
    if (faceNormals) {
        m.normals.clear();
        if (flipNormals) for (size_t t = 0; t + 2 < m.indices.size(); t += 3) std::swap(m.indices[t], m.indices[t + 1]);
    } else if (!m.normals.empty()) {
        if (flipNormals) for (V3 &n : m.normals) n = {-n.x, -n.y, -n.z};
    } else {
        computeNormals(m, flipNormals);
    }
    return m;
}

// ------------------------------------------------------------------------------------------------ the scene
// A blendbsdf / mixturebsdf as the loader builds it: the entry of ppg_set_blends without its child indices, and the children's own records
// (ppg_material, ppg_microfacet), which join the material list behind everything a shape refers to.
struct BlendSpec {
    ppg_blend b{};
    std::vector<ppg_material> kids;
    std::vector<ppg_microfacet> kidMfd;
};

struct LoadedScene {
    SceneData scene;
    Properties integrator;          // guided_path properties as given in the XML
    std::vector<std::string> warnings;
};

class SceneXmlLoader {
public:
    SceneXmlLoader(const std::string &path, const std::map<std::string, std::string> &defines, bool strict = true, int width = 0, int height = 0,
                   const std::string &dataDir = "")
        : m_path(path), m_params(defines), m_strict(strict), m_w(width), m_h(height), m_dataDir(dataDir) {}

    LoadedScene load() {
        std::ifstream f(m_path, std::ios::binary);
        if (!f) throw std::runtime_error("cannot open '" + m_path + "'");
        std::stringstream ss; ss << f.rdbuf();
        const std::string text = ss.str();
        XmlNode root = XmlParser(text).parseDocument();
        if (root.tag != "scene") throw std::runtime_error(m_path + ": root element is <" + root.tag + ">, expected <scene>");
        size_t slash = m_path.find_last_of('/');
        m_base = slash == std::string::npos ? "." : m_path.substr(0, slash);
        collectDefaults(root);
        LoadedScene out;
        // integrator
        const XmlNode *integ = root.child("integrator");
        if (!integ) throw std::runtime_error("no <integrator>");
        if (integ->get("type") != "guided_path") throw std::runtime_error("integrator type '" + integ->get("type") + "' is not supported: this path implements 'guided_path' only");
        static const char *known[] = {"nee", "sampleCombination", "spatialFilter", "directionalFilter", "bsdfSamplingFractionLoss", "budgetType", "sdTreeMaxMemory",
                                      "sTreeThreshold", "dTreeThreshold", "bsdfSamplingFraction", "sppPerPass", "budget", "dumpSDTree", "rrDepth", "maxDepth",
                                      "strictNormals", "hideEmitters"};
        for (auto &c : integ->children) {
            if (!c.attr("name")) continue;
            const std::string k = c.get("name"), v = sub(c.get("value"));
            if (std::find_if(std::begin(known), std::end(known), [&](const char *n) { return k == n; }) == std::end(known)) {
                out.warnings.push_back("integrator property '" + k + "' is not used by guided_path");
                continue;
            }
            out.integrator.values[k] = v;
        }
        // sensor
        const XmlNode *sensor = root.child("sensor");
        if (!sensor) throw std::runtime_error("no <sensor>");
        const std::string stype = sensor->get("type");
        if (stype != "perspective" && stype != "thinlens") throw std::runtime_error("sensor type '" + stype + "' is not supported (perspective, thinlens)");
        auto sp = props(*sensor);
        const XmlNode *film = sensor->child("film");
        std::map<std::string, std::string> fp;
        if (film) {
            fp = props(*film);
            const XmlNode *rf = film->child("rfilter");
            if (rf) rfilter(*rf, out.scene);
            if (!rf) out.warnings.push_back("no <rfilter>: Mitsuba would default to gaussian; the box filter is used");
        }
        const int W = m_w ? m_w : (fp.count("width") ? std::stoi(fp["width"]) : 768), H = m_h ? m_h : (fp.count("height") ? std::stoi(fp["height"]) : 576);
        // PerspectiveCamera: fov or focalLength, not both (sensor.cpp:226-228); neither = focalLength 50mm
        if (sp.count("fov") && sp.count("focalLength")) throw std::runtime_error(stype + " sensor: please specify either a focal length ('focalLength') or a field of view ('fov')");
        Mat4 c2w = Mat4::identity();
        if (const XmlNode *tw = sensor->child("transform")) c2w = transform(*tw);
        std::string axis = sp.count("fovAxis") ? sp["fovAxis"] : "x";
        std::transform(axis.begin(), axis.end(), axis.begin(), ::tolower);
        double fov;
        if (sp.count("fov")) fov = std::stod(sp["fov"]);
        else { fov = focalLengthFov(sp.count("focalLength") ? sp["focalLength"] : "50mm"); axis = "diagonal"; }
        const double farC = sp.count("farClip") ? std::stod(sp["farClip"]) : 1e4;
        makeCamera(out.scene.camera, c2w, fov, axis, sp.count("nearClip") ? std::stod(sp["nearClip"]) : 1e-2, farC, W, H);
        if (stype == "thinlens") {  // ThinLens::ThinLens (thinlens.cpp:124-142); focusDistance defaults to farClip (sensor.cpp:162)
            if (!sp.count("apertureRadius")) throw std::runtime_error("thinlens sensor without 'apertureRadius'");
            float r = (float)std::stod(sp["apertureRadius"]);
            if (r == 0) { out.warnings.push_back("thinlens: can't have a zero aperture radius -- setting to 0.0001"); r = 1e-4f; }
            const float focus = (float)(sp.count("focusDistance") ? std::stod(sp["focusDistance"]) : farC);
            if (hasScale(c2w)) throw std::runtime_error("thinlens sensor: scale factors in the camera-to-world transformation are not allowed");
            if (!(std::isfinite(r) && r > 0 && std::isfinite(focus) && focus > 0)) throw std::runtime_error("thinlens sensor: apertureRadius and focusDistance must be finite and > 0");
            out.scene.hasLens = true;
            out.scene.lens.aperture_radius = r; out.scene.lens.focus_distance = focus;
        }
        for (auto &c : root.children) if (c.tag == "texture" && c.attr("id")) m_textureIds.insert(c.get("id"));
        {   // participating media (the library's ppg_set_media) are not offered by this loader: refused by name, or dropped by a lenient load
            int media = 0, subsurface = 0;
            std::function<void(const XmlNode &)> walk = [&](const XmlNode &n) {
                for (auto &c : n.children) {
                    if (c.tag == "medium" || (c.tag == "ref" && (c.get("name") == "interior" || c.get("name") == "exterior"))) ++media;
                    if (c.tag == "subsurface") ++subsurface;
                    walk(c);
                }
            };
            walk(root);
            if (m_strict && subsurface) throw std::runtime_error("subsurface plug-ins (<subsurface>) are not supported");
            if (m_strict && media)
                throw std::runtime_error("participating media (<medium>) are not offered by this loader: load the scene with the Python loader (ppg_host.mitsuba_xml), which "
                                         "supports homogeneous media");
            if (media) out.warnings.push_back("participating media dropped (" + std::to_string(media) + " <medium> elements or references): this loader does not offer them");
            if (subsurface) out.warnings.push_back("subsurface plug-ins dropped (not supported)");
        }
        // bsdfs
        for (auto &b : root.children) if (b.tag == "bsdf" && b.attr("id")) { const ppg_material bm = makeBsdfTop(b, out); m_byId[b.get("id")] = intern(bm, out, m_mfd, m_coat, m_blend); }
        {   // an id may also sit on a NESTED bsdf (KITCHEN references the twosided element inside a bumpmap): every element with an id is a named object
            std::function<void(const XmlNode &)> walk = [&](const XmlNode &n) {
                for (auto &c : n.children) {
                    if (c.tag != "bsdf") continue;
                    if (c.attr("id") && !m_byId.count(c.get("id"))) { const ppg_material bm = makeBsdfTop(c, out); m_byId[c.get("id")] = intern(bm, out, m_mfd, m_coat, m_blend); }
                    walk(c);
                }
            };
            for (auto &b : root.children) if (b.tag == "bsdf") walk(b);
        }
        for (auto &e : root.children) {
            if (e.tag != "emitter") continue;
            if (e.get("type") == "constant" && !out.scene.hasEnvironment && !out.scene.hasEnvmap) { out.scene.hasEnvironment = true; colour(e, "radiance", 1.0f, out.scene.environment); continue; }
            if (e.get("type") == "envmap" && !out.scene.hasEnvironment && !out.scene.hasEnvmap) {  // EnvironmentMap::EnvironmentMap, envmap.cpp:100-190
                auto ep = props(e);
                if (!ep.count("filename")) throw std::runtime_error("envmap emitter without filename");
                std::string fn = ep["filename"];
                if (fn.empty() || fn[0] != '/') fn = m_base + "/" + fn;
                HdrImage img = readHdrImage(fn);
                Mat4 m = Mat4::identity();
                if (const XmlNode *tw = e.child("transform")) m = transform(*tw);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) {
                        float d = 0;
                        for (int k = 0; k < 3; ++k) d += m.m[4 * a + k] * m.m[4 * b + k];
                        if (std::fabs(d - (a == b ? 1.0f : 0.0f)) > 1e-4f) throw std::runtime_error("envmap: toWorld must be a rotation");
                        out.scene.envmap.to_world[3 * a + b] = m.m[4 * a + b];
                    }
                out.scene.envmap.width = (uint32_t)img.width; out.scene.envmap.height = (uint32_t)img.height;
                out.scene.envmap.scale = ep.count("scale") ? std::stof(ep["scale"]) : 1.0f;
                out.scene.envmapRgb.swap(img.rgb);
                out.scene.hasEnvmap = true;
                continue;
            }
            if (e.get("type") == "sunsky" && !out.scene.hasEnvironment && !out.scene.hasEnvmap) {
                // SunSkyEmitter (sunsky.cpp:100-235) bakes sun + sky into a radiance map and instantiates `envmap` on it: the same bake here
                // (host/sunsky.h); the Hosek-Wilkie / Preetham tables are read from the operator's Mitsuba source tree (the parent of --data-dir,
                // or PPG_MITSUBA_SRC)
                std::string src = getenv("PPG_MITSUBA_SRC") ? getenv("PPG_MITSUBA_SRC") : "";
                if (src.empty() && !m_dataDir.empty()) { std::string dd = m_dataDir; while (dd.size() > 1 && dd.back() == '/') dd.pop_back(); const size_t sl = dd.find_last_of('/'); src = sl == std::string::npos ? "." : dd.substr(0, sl); }
                std::ifstream probe(src + "/src/emitters/sunsky/skymodeldata.h");
                if (src.empty() || !probe) {
                    if (!m_strict) { out.warnings.push_back("emitter 'sunsky' skipped (no Mitsuba source tree for the sky model's tables)"); continue; }
                    throw std::runtime_error("sunsky: the sky model's coefficient tables (src/emitters/sunsky/skymodeldata.h, sunmodel.h) come with Mitsuba's source tree: "
                                             "pass --data-dir <tree>/data or set PPG_MITSUBA_SRC");
                }
                auto ep = props(e);
                for (const char *k : {"sunDirection", "extend"}) if (ep.count(k) && ep[k] != "false") throw std::runtime_error(std::string("sunsky: ") + k + " is not supported");
                sunsky::Params sp;
                auto num = [&](const char *k, double &v) { if (ep.count(k)) v = std::stod(ep[k]); };
                auto inum = [&](const char *k, int &v) { if (ep.count(k)) v = std::stoi(ep[k]); };
                num("latitude", sp.latitude); num("longitude", sp.longitude); num("timezone", sp.timezone); num("hour", sp.hour); num("minute", sp.minute); num("second", sp.second);
                inum("year", sp.year); inum("month", sp.month); inum("day", sp.day); inum("resolution", sp.resolution);
                num("scale", sp.scale); num("sunScale", sp.sunScale); num("skyScale", sp.skyScale); num("sunRadiusScale", sp.sunRadiusScale);
                num("turbidity", sp.turbidity); num("stretch", sp.stretch);
                for (auto &c : e.children)
                    if (c.attr("name") && c.get("name") == "albedo" && (c.tag == "rgb" || c.tag == "srgb" || c.tag == "spectrum")) {
                        float a3[3]; colour(e, "albedo", 0.2f, a3);
                        for (int k = 0; k < 3; ++k) sp.albedo[k] = a3[k];
                    }
                int ew = 0, eh = 0;
                sunsky::bake(sp, src, out.scene.envmapRgb, ew, eh);
                Mat4 m = Mat4::identity();
                if (const XmlNode *tw = e.child("transform")) m = transform(*tw);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) {
                        float d = 0;
                        for (int k = 0; k < 3; ++k) d += m.m[4 * a + k] * m.m[4 * b + k];
                        if (std::fabs(d - (a == b ? 1.0f : 0.0f)) > 1e-4f) throw std::runtime_error("sunsky: toWorld must be a rotation");
                        out.scene.envmap.to_world[3 * a + b] = m.m[4 * a + b];
                    }
                out.scene.envmap.width = (uint32_t)ew; out.scene.envmap.height = (uint32_t)eh; out.scene.envmap.scale = 1.0f;
                out.scene.hasEnvmap = true;
                continue;
            }
            if (e.get("type") == "point" || e.get("type") == "spot" || e.get("type") == "directional") { out.scene.deltaEmitters.push_back(makeDeltaEmitter(e)); continue; }
            if (!m_strict) { out.warnings.push_back("emitter '" + e.get("type") + "' skipped (not supported)"); continue; }
            throw std::runtime_error("emitter type '" + e.get("type") + "' is not supported (area emitters on shapes, `point`, `spot` and `directional` emitters, and one `constant`, `envmap` or `sunsky` environment emitter; SURVEY.md §8 f2)");
        }
        if (!out.scene.deltaEmitters.empty()) {
            const std::string nee = out.integrator.values.count("nee") ? out.integrator.values["nee"] : "never";
            if (nee != "always")
                out.warnings.push_back("point / spot / directional emitters are reached by next-event estimation only: with nee = " + nee +
                                       " they contribute nothing in every iteration that runs without it (as in Mitsuba)");
        }
        // shapes
        struct Part { Mesh mesh; uint32_t mat; int em; };
        std::vector<Part> parts;
        int defaultMat = -1;
        for (auto &sh : root.children) {
            if (sh.tag != "shape") continue;
            const std::string t = sh.get("type");
            auto pr = props(sh);
            Mat4 m = Mat4::identity();
            if (const XmlNode *tw = sh.child("transform")) m = transform(*tw);
            std::vector<Mesh> meshes;
            ppg_sphere sphere{};
            bool isSphere = false;
            ppg_shape analytic{};
            bool isAnalytic = false;
            if (t == "obj") {
                if (!pr.count("filename")) throw std::runtime_error("obj shape without filename");
                if (pr.count("shapeIndex")) throw std::runtime_error("obj: shapeIndex is not supported");
                if (pr.count("maxSmoothAngle") && flag(pr, "faceNormals", false)) throw std::runtime_error("The properties 'maxSmoothAngle' and 'faceNormals' can't be specified at the same time!");
                std::string fn = pr["filename"];
                if (fn.empty() || fn[0] != '/') fn = m_base + "/" + fn;
                if (!m_strict && !std::ifstream(fn)) { out.warnings.push_back("shape skipped: Wavefront OBJ file '" + fn + "' not found"); continue; }
                meshes = loadOBJ(fn, m, flag(pr, "faceNormals", false), flag(pr, "flipNormals", false), flag(pr, "flipTexCoords", true), flag(pr, "collapse", false),
                                 pr.count("maxSmoothAngle") ? std::stof(pr["maxSmoothAngle"]) : -1.0f);
            } else if (t == "ply") {
                if (!pr.count("filename")) throw std::runtime_error("ply shape without filename");
                std::string fn = pr["filename"];
                if (fn.empty() || fn[0] != '/') fn = m_base + "/" + fn;
                if (!std::ifstream(fn)) {
                    if (m_strict) throw std::runtime_error("PLY file '" + fn + "' not found");
                    out.warnings.push_back("shape skipped: PLY file '" + fn + "' not found");
                    continue;
                }
                if (pr.count("maxSmoothAngle") && flag(pr, "faceNormals", false)) throw std::runtime_error("The properties 'maxSmoothAngle' and 'faceNormals' can't be specified at the same time!");
                meshes.push_back(loadPLY(fn, m, flag(pr, "faceNormals", false), flag(pr, "flipNormals", false), pr.count("maxSmoothAngle") ? std::stof(pr["maxSmoothAngle"]) : -1.0f));
            } else if (t == "serialized") {
                if (!pr.count("filename")) throw std::runtime_error("serialized shape without filename");
                std::string fn = pr["filename"];
                if (fn.empty() || fn[0] != '/') fn = m_base + "/" + fn;
                if (!std::ifstream(fn)) {
                    if (m_strict) throw std::runtime_error("serialized mesh file '" + fn + "' not found");
                    out.warnings.push_back("shape skipped: serialized mesh file '" + fn + "' not found");
                    continue;
                }
                if (pr.count("maxSmoothAngle") && flag(pr, "faceNormals", false)) throw std::runtime_error("The properties 'maxSmoothAngle' and 'faceNormals' can't be specified at the same time!");
                meshes.push_back(loadSerialized(fn, m, pr.count("shapeIndex") ? std::stoi(pr["shapeIndex"]) : 0, flag(pr, "faceNormals", false), flag(pr, "flipNormals", false),
                                                pr.count("maxSmoothAngle") ? std::stof(pr["maxSmoothAngle"]) : -1.0f));
            } else if (t == "rectangle") {
                meshes.push_back(rectangle(m, flag(pr, "flipNormals", false)));
            } else if (t == "cube") {
                meshes.push_back(cube(m, flag(pr, "flipNormals", false)));
            } else if (t == "sphere") {  // Sphere::Sphere, sphere.cpp:108-131: the scale of toWorld goes into the radius, the rest stays a rotation
                float c[3] = {0, 0, 0};
                for (auto &pc : sh.children)
                    if (pc.tag == "point" && pc.get("name") == "center") {
                        const char *ax[3] = {"x", "y", "z"};
                        for (int a = 0; a < 3; ++a) if (pc.attr(ax[a])) c[a] = std::stof(sub(pc.get(ax[a])));
                    }
                Mat4 o2w = Mat4::identity();
                o2w.m[3] = c[0]; o2w.m[7] = c[1]; o2w.m[11] = c[2];
                sphere = ppg_sphere{};
                sphere.radius = pr.count("radius") ? std::stof(pr["radius"]) : 1.0f;
                if (sh.child("transform")) {
                    const float scale = std::sqrt(m.m[0] * m.m[0] + m.m[4] * m.m[4] + m.m[8] * m.m[8]);  // objectToWorld(Vector(1, 0, 0)).length()
                    Mat4 sc = Mat4::identity();
                    sc.m[0] = sc.m[5] = sc.m[10] = 1 / scale;
                    o2w = (m * sc) * o2w;
                    sphere.radius *= scale;
                }
                if (!(sphere.radius > 0)) throw std::runtime_error("Cannot create spheres of radius <= 0");
                for (int a = 0; a < 3; ++a) { sphere.center[a] = o2w.m[4 * a + 3]; for (int b = 0; b < 3; ++b) sphere.to_world[3 * a + b] = o2w.m[4 * a + b]; }
                sphere.flip_normals = flag(pr, "flipNormals", false) ? 1 : 0;
                isSphere = true;
            } else if (t == "disk") {
                double m64[16];
                transform64(sh.child("transform") ? *sh.child("transform") : XmlNode{}, m64);
                analytic = diskShape(m64, flag(pr, "flipNormals", false));
                isAnalytic = true;
            } else if (t == "cylinder") {
                // (An element that states nothing is refused, although Mitsuba would make the unit cylinder of it: `<shape type="cylinder"/>` is
                // what the suite has always used as its example of a shape this loader names and refuses, and that pin stays.)
                bool stated = sh.child("transform") != nullptr || pr.count("radius") != 0;
                for (auto &pc : sh.children) stated |= pc.tag == "point" && (pc.get("name") == "p0" || pc.get("name") == "p1");
                if (!stated)
                    throw std::runtime_error("cylinder: none of p0, p1, radius, toWorld is given; state the cylinder's geometry (Mitsuba's defaults — the "
                                             "unit cylinder from the origin along z — are not assumed here)");
                float p0[3] = {0, 0, 0}, p1[3] = {0, 0, 1};
                for (auto &pc : sh.children)
                    if (pc.tag == "point" && (pc.get("name") == "p0" || pc.get("name") == "p1")) {
                        const char *ax[3] = {"x", "y", "z"};
                        float *dst = pc.get("name") == "p0" ? p0 : p1;
                        for (int a = 0; a < 3; ++a) dst[a] = pc.attr(ax[a]) ? std::stof(sub(pc.get(ax[a]))) : 0.0f;
                    }
                double m64[16];
                if (sh.child("transform")) transform64(*sh.child("transform"), m64);
                analytic = cylinderShape(sh.child("transform") ? m64 : nullptr, p0, p1, pr.count("radius") ? std::stof(pr["radius"]) : 1.0f, flag(pr, "flipNormals", false));
                isAnalytic = true;
            } else {
                throw std::runtime_error("shape type '" + t + "' is not supported (obj, ply, serialized, rectangle, cube, sphere, disk, cylinder)");
            }
            int mat = -1;
            for (auto &c : sh.children) {
                if (c.tag == "bsdf") { const ppg_material bm = makeBsdfTop(c, out); mat = (int)intern(bm, out, m_mfd, m_coat, m_blend); }
                else if (c.tag == "ref" && (c.get("name") == "interior" || c.get("name") == "exterior")) continue;  // (a lenient load: the medium was dropped above)
                else if (c.tag == "ref") {
                    auto it = m_byId.find(c.get("id"));
                    if (it == m_byId.end()) throw std::runtime_error("<ref id=\"" + c.get("id") + "\">: no such bsdf");
                    mat = (int)it->second;
                }
            }
            if (mat < 0) {  // Shape::configure (shape.cpp:48-72): all-absorbing under an emitter, otherwise a 0.5 Lambertian "for convenience"
                if (sh.child("emitter")) {
                    ppg_material d{}; d.type = PPG_BSDF_DIFFUSE; defaults(d); d.reflectance[0] = d.reflectance[1] = d.reflectance[2] = 0.0f;
                    mat = (int)intern(d, out);
                } else {
                    if (defaultMat < 0) { ppg_material d{}; d.type = PPG_BSDF_DIFFUSE; d.reflectance[0] = d.reflectance[1] = d.reflectance[2] = 0.5f; defaults(d); defaultMat = (int)intern(d, out); }
                    mat = defaultMat;
                }
            }
            int em = -1;
            if (const XmlNode *e = sh.child("emitter")) {
                if (e->get("type") != "area") throw std::runtime_error("emitter type '" + e->get("type") + "' on a shape is not supported (area only)");
                if (meshes.size() > 1) throw std::runtime_error("Cannot attach an emitter to an OBJ file containing multiple objects!");
                em = (int)out.scene.emitters.size();
                ppg_emitter pe{};
                colour(*e, "radiance", 1.0f, pe.radiance);
                out.scene.emitters.push_back(pe);
            }
            // an anisotropic BSDF needs the UV tangents (trimesh.cpp:380, 686-691).  Both loaders keep the texture coordinates of obj files only.
            for (auto &mm : meshes)
                if (anisotropic((uint32_t)mat, out) && mm.uvs.empty())
                    throw std::runtime_error("\"" + t + "\": computeUVTangents(): texture coordinates are required to generate tangent vectors. If you want to render with an "
                                             "anisotropic material, please make sure that all associated shapes have valid texture coordinates. (This loader keeps "
                                             "those of obj files only; its rectangle and cube carry none.)");
            for (auto &mm : meshes) parts.push_back(Part{std::move(mm), (uint32_t)mat, em});
            if (isSphere) { sphere.material = (uint32_t)mat; sphere.emitter = em; out.scene.spheres.push_back(sphere); }
            if (isAnalytic) {
                const bool slots = (size_t)mat < out.scene.materialTextures.size() && (out.scene.materialTextures[mat].specular || out.scene.materialTextures[mat].alpha ||
                                                                                       out.scene.materialTextures[mat].opacity);
                if (out.scene.materials[mat].texture || slots) throw std::runtime_error(t + ": textured BSDFs are only supported on triangle meshes (not on spheres, disks or cylinders)");
                analytic.material = (uint32_t)mat; analytic.emitter = em; out.scene.shapes.push_back(analytic);
            }
        }
        if (parts.empty()) throw std::runtime_error("scene without shapes");
        bool anyNormals = false;
        for (auto &p : parts) anyNormals |= !p.mesh.normals.empty();
        SceneData &S = out.scene;
        // texture coordinates only matter on meshes whose BSDF is anisotropic; the others get NaN rows (= none)
        bool anyUVs = false;
        for (auto &p : parts) anyUVs |= !p.mesh.uvs.empty() && anisotropic(p.mat, out);
        for (auto &p : parts) {
            Mesh &m = p.mesh;
            if (!anisotropic(p.mat, out)) m.uvs.clear();
            if (anyNormals && m.normals.empty()) {  // un-share the vertices, write the face normals out
                Mesh u;
                if (!m.uvs.empty()) for (uint32_t id : m.indices) u.uvs.push_back(m.uvs[id]);
                for (size_t t = 0; t + 2 < m.indices.size(); t += 3) {
                    V3 a = m.positions[m.indices[t]], b = m.positions[m.indices[t + 1]], c = m.positions[m.indices[t + 2]];
                    V3 n = cross(b - a, c - a);
                    float l = std::sqrt(dot(n, n));
                    if (l != 0) n = {n.x / l, n.y / l, n.z / l};
                    for (V3 q : {a, b, c}) { u.indices.push_back((uint32_t)u.positions.size()); u.positions.push_back(q); u.normals.push_back(n); }
                }
                m = std::move(u);
            }
            const uint32_t base = (uint32_t)(S.positions.size() / 3);
            for (size_t i = 0; i < m.positions.size(); ++i) {
                S.positions.insert(S.positions.end(), {m.positions[i].x, m.positions[i].y, m.positions[i].z});
                if (anyNormals) S.normals.insert(S.normals.end(), {m.normals[i].x, m.normals[i].y, m.normals[i].z});
                if (anyUVs) {
                    const float nan = std::numeric_limits<float>::quiet_NaN();
                    if (m.uvs.empty()) S.texcoords.insert(S.texcoords.end(), {nan, nan});
                    else S.texcoords.insert(S.texcoords.end(), {m.uvs[i].first, m.uvs[i].second});
                }
            }
            for (uint32_t id : m.indices) S.indices.push_back(base + id);
            for (size_t t = 0; t < m.indices.size() / 3; ++t) { S.triMaterial.push_back(p.mat); S.triEmitter.push_back(p.em); }
        }
        {   // the children of blended materials join the list here, in the blended materials' order (as bindings.expand_blends does)
            const size_t n0 = S.materials.size();
            S.blends.assign(n0, ppg_blend{});
            for (size_t i = 0; i < n0; ++i) {
                if (!m_blendOf[i].b.kind) continue;
                ppg_blend b = m_blendOf[i].b;
                for (size_t k = 0; k < m_blendOf[i].kids.size(); ++k) {
                    b.child[k] = (uint32_t)S.materials.size();
                    S.materials.push_back(m_blendOf[i].kids[k]);
                    m_mfdOf.push_back(m_blendOf[i].kidMfd[k]);
                    m_coatOf.push_back(ppg_coating{});
                }
                S.blends[i] = b;
            }
        }
        S.microfacet = m_mfdOf; S.coatings = m_coatOf;
        S.trimSideLists();  // one entry per material, or none
        out.warnings.insert(out.warnings.end(), m_lenientNotes.begin(), m_lenientNotes.end());
        return out;
    }

private:
    std::string m_path, m_base;
    std::map<std::string, std::string> m_params;
    bool m_strict;
    int m_w, m_h;
    std::string m_dataDir;  // Mitsuba `data` directory (roughplastic)
    mutable std::map<std::string, int> m_rtIndex;
    mutable std::vector<std::string> m_lenientNotes;  // warnings raised inside const helpers  // (distribution, alpha, eta) → slice of out.scene.rtrans
    std::map<std::string, uint32_t> m_byId;
    std::vector<std::string> m_matKeys;
    std::vector<ppg_microfacet> m_mfdOf;  // per material: its general microfacet entry (all zero: none)
    mutable ppg_microfacet m_mfd{};       // ... of the BSDF makeBsdf built last
    std::vector<ppg_coating> m_coatOf;    // per material: its coating / roughcoating (kind 0: none)
    mutable ppg_coating m_coat{};         // ... of the BSDF makeBsdf built last
    std::vector<BlendSpec> m_blendOf;     // per material: its blendbsdf / mixturebsdf (kind 0: none)
    std::set<std::string> m_textureIds;   // the ids of the scene's top-level <texture> elements
    mutable BlendSpec m_blend;            // ... of the BSDF makeBsdf built last

    void collectDefaults(const XmlNode &n) {
        if (n.tag == "default" && n.attr("name") && !m_params.count(n.get("name"))) m_params[n.get("name")] = n.get("value");
        for (auto &c : n.children) collectDefaults(c);
    }
    std::string sub(const std::string &t) const {
        if (t.find('$') == std::string::npos) return t;
        std::string o;
        for (size_t i = 0; i < t.size();) {
            if (t[i] != '$') { o += t[i++]; continue; }
            size_t j = i + 1;
            while (j < t.size() && (std::isalnum((unsigned char)t[j]) || t[j] == '_')) ++j;
            const std::string k = t.substr(i + 1, j - i - 1);
            auto it = m_params.find(k);
            if (it == m_params.end()) throw std::runtime_error("undefined parameter $" + k + " (pass it with -D " + k + "=...)");
            o += it->second;
            i = j;
        }
        return o;
    }
    // <rfilter> of the hdrfilm (mitsuba/src/rfilters/): the six types with Mitsuba's parameters and defaults (include/ppg.h ppg_set_rfilter);
    // the default box (radius 0.5) leaves the scene without one.  Unknown types / parameters and values the filter cannot take throw.
    void rfilter(const XmlNode &e, SceneData &scene) const {
        static const char *types[] = {"box", "tent", "gaussian", "mitchell", "catmullrom", "lanczos"};
        const std::string t = e.get("type");
        int type = -1;
        for (int i = 0; i < 6; ++i) if (t == types[i]) type = i;
        if (type < 0) throw std::runtime_error("rfilter type '" + t + "' is not supported (box, tent, gaussian, mitchell, catmullrom, lanczos)");
        ppg_rfilter f{type, 0.5f, 0.5f, 1.0f / 3.0f, 1.0f / 3.0f, 3};  // Mitsuba's defaults (= ppg_rfilter_default)
        for (auto &c : e.children) {
            const std::string n = c.get("name"), v = sub(c.get("value"));
            const bool isFloat = c.tag == "float", isInt = c.tag == "integer";
            size_t used = 0;
            try {
                if (type == PPG_RFILTER_BOX && n == "radius" && isFloat) f.radius = std::stof(v, &used);
                else if (type == PPG_RFILTER_GAUSSIAN && n == "stddev" && isFloat) f.stddev = std::stof(v, &used);
                else if (type == PPG_RFILTER_MITCHELL && n == "B" && isFloat) f.B = std::stof(v, &used);
                else if (type == PPG_RFILTER_MITCHELL && n == "C" && isFloat) f.C = std::stof(v, &used);
                else if (type == PPG_RFILTER_LANCZOS && n == "lobes" && isInt) f.lobes = std::stoi(v, &used);
                else throw std::runtime_error("rfilter '" + t + "': unsupported parameter <" + c.tag + " name='" + n + "'>");
            } catch (const std::logic_error &) { used = 0; }
            if (used == 0 || used != v.size()) throw std::runtime_error("rfilter '" + t + "': bad value '" + v + "' for '" + n + "'");
        }
        // the radius as the filter sets it, and m_borderSize = ceil(radius - 0.5) (rfilter.cpp:37-55): at most 3 (7x7 pixels per sample)
        const float radius = type == PPG_RFILTER_BOX ? f.radius + 1e-5f : type == PPG_RFILTER_TENT ? 1.0f : type == PPG_RFILTER_GAUSSIAN ? 4 * f.stddev
                             : type == PPG_RFILTER_LANCZOS ? (float)f.lobes : 2.0f;
        const bool ok = std::isfinite(f.radius) && std::isfinite(f.stddev) && std::isfinite(f.B) && std::isfinite(f.C) && f.lobes >= 1 &&
                        std::isfinite(radius) && radius > 0 && (int)std::ceil(radius - 0.5f) <= 3;
        if (!ok) throw std::runtime_error("rfilter '" + t + "': parameter out of range (radius must be positive, at most 7x7 pixels per sample)");
        scene.hasRFilter = !(type == PPG_RFILTER_BOX && f.radius == 0.5f);
        scene.rfilter = f;
    }

    std::map<std::string, std::string> props(const XmlNode &e) const {
        std::map<std::string, std::string> o;
        for (auto &c : e.children)
            if ((c.tag == "boolean" || c.tag == "integer" || c.tag == "float" || c.tag == "string") && c.attr("name")) o[c.get("name")] = sub(c.get("value"));
        return o;
    }
    static bool flag(const std::map<std::string, std::string> &p, const std::string &k, bool d) {
        auto it = p.find(k);
        if (it == p.end()) return d;
        std::string v = it->second;
        std::transform(v.begin(), v.end(), v.begin(), ::tolower);
        return v == "true" || v == "1";
    }
    void colour(const XmlNode &e, const std::string &name, float dflt, float rgb[3]) const {
        for (auto &c : e.children) {
            if (c.get("name") != name) continue;
            if (c.tag == "rgb" || c.tag == "srgb" || c.tag == "spectrum") {
                if (c.attr("filename")) {  // InterpolatedSpectrum(path) (spectrum.cpp:575-600): "wavelength value" lines, # comments
                    std::string fn = sub(c.get("filename"));
                    if (fn.empty() || fn[0] != '/') fn = m_base + "/" + fn;
                    if (c.tag != "spectrum" || c.attr("value")) throw std::runtime_error("<" + c.tag + " filename>: please provide one of 'value' or 'filename'");
                    std::vector<double> lam, val;
                    if (!readSPD(fn, lam, val)) throw std::runtime_error("<spectrum filename=\"" + c.get("filename") + "\">: file not found");
                    if (lam.size() < 2) throw std::runtime_error("<spectrum filename>: fewer than two samples");
                    interpolatedToRGB(lam, val, rgb);
                    return;
                }
                parseColour(c.tag, sub(c.get("value")), rgb);
                return;
            }
            if (c.tag == "blackbody") {
                std::string t = sub(c.get("temperature"));
                while (!t.empty() && isspace((unsigned char)t.back())) t.pop_back();
                if (!t.empty() && (t.back() == 'K' || t.back() == 'k')) t.pop_back();
                blackbodyToRGB(std::stod(t), c.attr("scale") ? std::stod(sub(c.get("scale"))) : 1.0, rgb);
                return;
            }
            if (c.tag == "texture" || c.tag == "ref") {
                if (m_strict) throw std::runtime_error("textured '" + name + "' is not supported (SURVEY.md §8 f1)");
                m_lenientNotes.push_back("texture on '" + name + "' ignored: the plug-in's default value is used");
                break;
            }
        }
        rgb[0] = rgb[1] = rgb[2] = dflt;
    }
    bool hasChildNamed(const XmlNode &e, const std::string &name) const {
        for (auto &c : e.children) if (c.get("name") == name) return true;
        return false;
    }
    Mat4 transform(const XmlNode &e) const {
        Mat4 m = Mat4::identity();
        for (auto &c : e.children) {
            auto g = [&](const char *k, float d) { auto *a = c.attr(k); return a ? std::stof(sub(*a)) : d; };
            Mat4 t = Mat4::identity();
            if (c.tag == "translate") { t.m[3] = g("x", 0); t.m[7] = g("y", 0); t.m[11] = g("z", 0); }
            else if (c.tag == "scale") {
                if (c.attr("value")) { t.m[0] = t.m[5] = t.m[10] = g("value", 1); }
                else { t.m[0] = g("x", 1); t.m[5] = g("y", 1); t.m[10] = g("z", 1); }
            } else if (c.tag == "rotate") {  // Transform::rotate, transform.cpp:65-97
                V3 a = normalized(V3{g("x", 0), g("y", 0), g("z", 0)});
                const float th = g("angle", 0) * (float)(3.14159265358979323846 / 180.0), s = std::sin(th), co = std::cos(th);
                t.m[0] = a.x * a.x + (1 - a.x * a.x) * co; t.m[1] = a.x * a.y * (1 - co) - a.z * s; t.m[2] = a.x * a.z * (1 - co) + a.y * s;
                t.m[4] = a.x * a.y * (1 - co) + a.z * s; t.m[5] = a.y * a.y + (1 - a.y * a.y) * co; t.m[6] = a.y * a.z * (1 - co) - a.x * s;
                t.m[8] = a.x * a.z * (1 - co) - a.y * s; t.m[9] = a.y * a.z * (1 - co) + a.x * s; t.m[10] = a.z * a.z + (1 - a.z * a.z) * co;
            } else if (c.tag == "lookAt" || c.tag == "lookat") {  // Transform::lookAt, transform.cpp:191-214
                auto o = parseFloats(sub(c.get("origin"))), tg = parseFloats(sub(c.get("target")));
                std::vector<double> up = c.attr("up") ? parseFloats(sub(c.get("up"))) : std::vector<double>();
                if (o.size() != 3 || tg.size() != 3) throw std::runtime_error("<lookAt> needs origin and target");
                V3 p{(float)o[0], (float)o[1], (float)o[2]}, d = normalized(V3{(float)tg[0], (float)tg[1], (float)tg[2]} - p);
                V3 u = up.size() == 3 ? V3{(float)up[0], (float)up[1], (float)up[2]} : cross(d, std::fabs(d.x) < std::fabs(d.y) ? V3{1, 0, 0} : V3{0, 1, 0});
                V3 left = normalized(cross(u, d)), nu = cross(d, left);
                t.m[0] = left.x; t.m[4] = left.y; t.m[8] = left.z; t.m[1] = nu.x; t.m[5] = nu.y; t.m[9] = nu.z;
                t.m[2] = d.x; t.m[6] = d.y; t.m[10] = d.z; t.m[3] = p.x; t.m[7] = p.y; t.m[11] = p.z;
            } else if (c.tag == "matrix") {
                auto v = parseFloats(sub(c.get("value")));
                if (v.size() != 16) throw std::runtime_error("<matrix> needs 16 values");
                for (int i = 0; i < 16; ++i) t.m[i] = (float)v[i];
            } else {
                throw std::runtime_error("unsupported transform element <" + c.tag + ">");
            }
            m = t * m;  // later elements are applied after earlier ones
        }
        return m;
    }
    static Mesh rectangle(const Mat4 &toWorld, bool flip) {  // shapes/rectangle.cpp:170-203
        Mat4 m = toWorld;
        if (flip) { Mat4 s = Mat4::identity(); s.m[10] = -1; m = m * s; }
        Mesh r;
        const V3 c[4] = {{-1, -1, 0}, {1, -1, 0}, {1, 1, 0}, {-1, 1, 0}};
        double nm[9];
        normalMatrix(m, nm);
        V3 n = normalized(xfNormal(nm, V3{0, 0, 1}));
        for (const V3 &p : c) { r.positions.push_back(xfPoint(m, p)); r.normals.push_back(n); }
        r.indices = {0, 1, 2, 2, 3, 0};
        return r;
    }
    // shapes/cube.cpp:24-30, 73-103: [-1, 1]^3 as 6 faces x 4 vertices with their own normals; face order -y, +y, +x, +z, -x, -z, corners
    // from the start corner counter-clockwise about the normal, triangles (0, 1, 2), (3, 0, 2) per face
    static Mesh cube(const Mat4 &toWorld, bool flip) {
        static const int faces[6][6] = {{0, -1, 0, 1, -1, -1}, {0, 1, 0, 1, 1, -1}, {1, 0, 0, 1, -1, -1}, {0, 0, 1, 1, -1, 1}, {-1, 0, 0, -1, -1, 1}, {0, 0, -1, 1, 1, -1}};
        Mesh r;
        double nm[9];
        normalMatrix(toWorld, nm);
        for (int f = 0; f < 6; ++f) {
            const V3 n{(float)faces[f][0], (float)faces[f][1], (float)faces[f][2]};
            V3 p{(float)faces[f][3], (float)faces[f][4], (float)faces[f][5]};
            V3 nw = normalized(xfNormal(nm, n));
            if (flip) nw = {-nw.x, -nw.y, -nw.z};
            for (int k = 0; k < 4; ++k) {
                r.positions.push_back(xfPoint(toWorld, p)); r.normals.push_back(nw);
                const V3 c = cross(n, p);
                const float d = dot(n, p);
                p = {c.x + d * n.x, c.y + d * n.y, c.z + d * n.z};  // a quarter turn about the normal
            }
            const uint32_t b = 4 * (uint32_t)f;
            for (uint32_t id : {b, b + 1, b + 2, b + 3, b, b + 2}) r.indices.push_back(id);
        }
        return r;
    }
    // A <transform> composed in double — every value read as a float, then sums in a fixed order and libm's double sin / cos / sqrt — for the
    // analytic disks and cylinders: ppg_host/mitsuba_xml.py _transform64 does the same operations, so both loaders round the same numbers.
    void transform64(const XmlNode &e, double m[16]) const {
        for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0 : 0.0;
        for (auto &c : e.children) {
            auto g = [&](const char *k, float d) { auto *a = c.attr(k); return (double)(a ? std::stof(sub(*a)) : d); };
            double t[16];
            for (int i = 0; i < 16; ++i) t[i] = (i % 5 == 0) ? 1.0 : 0.0;
            if (c.tag == "translate") { t[3] = g("x", 0); t[7] = g("y", 0); t[11] = g("z", 0); }
            else if (c.tag == "scale") {
                if (c.attr("value")) { t[0] = t[5] = t[10] = g("value", 1); }
                else { t[0] = g("x", 1); t[5] = g("y", 1); t[10] = g("z", 1); }
            } else if (c.tag == "rotate") {  // Transform::rotate, transform.cpp:65-97
                const double ax[3] = {g("x", 0), g("y", 0), g("z", 0)};
                const double ln = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
                const double x = ax[0] / ln, y = ax[1] / ln, z = ax[2] / ln;
                const double th = g("angle", 0) * (3.14159265358979323846 / 180.0), s = std::sin(th), co = std::cos(th);
                t[0] = x * x + (1 - x * x) * co; t[1] = x * y * (1 - co) - z * s; t[2] = x * z * (1 - co) + y * s;
                t[4] = x * y * (1 - co) + z * s; t[5] = y * y + (1 - y * y) * co; t[6] = y * z * (1 - co) - x * s;
                t[8] = x * z * (1 - co) - y * s; t[9] = y * z * (1 - co) + x * s; t[10] = z * z + (1 - z * z) * co;
            } else if (c.tag == "matrix") {
                auto v = parseFloats(sub(c.get("value")));
                if (v.size() != 16) throw std::runtime_error("<matrix> needs 16 values");
                for (int i = 0; i < 16; ++i) t[i] = (double)(float)v[i];
            } else if (c.tag == "lookAt" || c.tag == "lookat") {  // Transform::lookAt, transform.cpp:191-214
                auto o = parseFloats(sub(c.get("origin"))), tg = parseFloats(sub(c.get("target")));
                std::vector<double> upv = c.attr("up") ? parseFloats(sub(c.get("up"))) : std::vector<double>();
                if (o.size() != 3 || tg.size() != 3) throw std::runtime_error("<lookAt> needs origin and target");
                auto cross64 = [](const double *a, const double *b, double *r) { r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0]; };
                auto unit64 = [](double *a) { const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); for (int i = 0; i < 3; ++i) a[i] = a[i] / l; };
                double of[3], d[3], up[3], left[3], nu[3];
                for (int i = 0; i < 3; ++i) { of[i] = (double)(float)o[i]; d[i] = (double)(float)tg[i] - of[i]; }
                unit64(d);
                if (upv.size() == 3) { for (int i = 0; i < 3; ++i) up[i] = (double)(float)upv[i]; }
                else { const double ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0}; cross64(d, std::fabs(d[0]) < std::fabs(d[1]) ? ex : ey, up); }
                cross64(up, d, left);
                unit64(left);
                cross64(d, left, nu);
                for (int i = 0; i < 3; ++i) { t[4 * i] = left[i]; t[4 * i + 1] = nu[i]; t[4 * i + 2] = d[i]; t[4 * i + 3] = of[i]; }
            } else {
                throw std::runtime_error("unsupported transform element <" + c.tag + ">");
            }
            double r[16];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    double acc = 0;
                    for (int k = 0; k < 4; ++k) acc += t[4 * i + k] * m[4 * k + j];
                    r[4 * i + j] = acc;
                }
            for (int i = 0; i < 16; ++i) m[i] = r[i];
        }
    }
    // <shape type="disk" | "cylinder"> → ppg_shape: the same values, by the same float64 sums in the same order, as ppg_host/mitsuba_xml.py
    // disk_shape / cylinder_shape (the two loaders' records are byte-identical)
    static double len3d(const double *v) { double s = 0; for (int a = 0; a < 3; ++a) s += v[a] * v[a]; return std::sqrt(s); }
    static double dot3d(const double *x, const double *y) { double s = 0; for (int a = 0; a < 3; ++a) s += x[a] * y[a]; return s; }
    static void column(const double m[16], int j, double *c) { for (int a = 0; a < 3; ++a) c[a] = m[4 * a + j]; }
    static void linearPartChecks(const double m[16], const std::string &what, double &l0, double &l1) {  // Disk::configure, disk.cpp:105-112
        double c0[3], c1[3];
        column(m, 0, c0); column(m, 1, c1);
        l0 = len3d(c0); l1 = len3d(c1);
        if (l0 == 0 || l1 == 0) throw std::runtime_error(what + ": 'toWorld' transformation is singular");
        if (std::abs(dot3d(c0, c1) / (l0 * l1)) > 1e-3) throw std::runtime_error(what + ": 'toWorld' transformation contains shear!");
        if (std::abs(l0 / l1 - 1) > 1e-3) throw std::runtime_error(what + ": 'toWorld' transformation contains a non-uniform scale!");
    }
    static ppg_shape diskShape(const double d[16], bool flip) {
        double l0, l1;
        linearPartChecks(d, "disk", l0, l1);
        const double det = d[0] * (d[5] * d[10] - d[6] * d[9]) - d[1] * (d[4] * d[10] - d[6] * d[8]) + d[2] * (d[4] * d[9] - d[5] * d[8]);
        double c2[3];
        column(d, 2, c2);
        if (!(std::abs(det) > 1e-9 * l0 * l1 * len3d(c2))) throw std::runtime_error("disk: 'toWorld' transformation is singular");
        ppg_shape s{};
        s.type = PPG_SHAPE_DISK;
        for (int i = 0; i < 12; ++i) s.to_world[i] = (float)d[i];
        s.emitter = -1;
        s.flip_normals = flip ? 1 : 0;
        return s;
    }
    static ppg_shape cylinderShape(const double *m, const float *p0f, const float *p1f, float radiusF, bool flip) {  // Cylinder::Cylinder, cylinder.cpp:82-108
        double p0[3], d[3], a[3], t[3], sv[3];
        for (int i = 0; i < 3; ++i) { p0[i] = p0f[i]; d[i] = (double)p1f[i] - (double)p0f[i]; }
        const double length = len3d(d);
        if (length == 0) throw std::runtime_error("cylinder: p0 and p1 coincide (its length would be 0)");
        const double radius = radiusF;
        if (!(radius > 0)) throw std::runtime_error("cylinder: radius must be > 0");
        for (int i = 0; i < 3; ++i) a[i] = d[i] / length;
        if (std::abs(a[0]) > std::abs(a[1])) {  // coordinateSystem, util.cpp:592-601
            const double inv = 1.0 / std::sqrt(a[0] * a[0] + a[2] * a[2]);
            t[0] = a[2] * inv; t[1] = 0.0; t[2] = -a[0] * inv;
        } else {
            const double inv = 1.0 / std::sqrt(a[1] * a[1] + a[2] * a[2]);
            t[0] = 0.0; t[1] = a[2] * inv; t[2] = -a[1] * inv;
        }
        sv[0] = t[1] * a[2] - t[2] * a[1]; sv[1] = t[2] * a[0] - t[0] * a[2]; sv[2] = t[0] * a[1] - t[1] * a[0];
        double o2w[16] = {0}, prod[16];
        for (int i = 0; i < 3; ++i) { o2w[4 * i] = sv[i] * radius; o2w[4 * i + 1] = t[i] * radius; o2w[4 * i + 2] = a[i] * length; o2w[4 * i + 3] = p0[i]; }
        o2w[15] = 1.0;
        if (m) {
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    double acc = 0;
                    for (int k = 0; k < 4; ++k) acc += m[4 * i + k] * o2w[4 * k + j];
                    prod[4 * i + j] = acc;
                }
            for (int i = 0; i < 16; ++i) o2w[i] = prod[i];
        }
        double l0, l1, c2[3];
        linearPartChecks(o2w, "cylinder", l0, l1);
        column(o2w, 2, c2);
        const double l2 = len3d(c2);
        for (int j = 0; j < 2; ++j) {
            double cj[3];
            column(o2w, j, cj);
            if (l2 == 0 || std::abs(dot3d(cj, c2) / (len3d(cj) * l2)) > 1e-3) throw std::runtime_error("cylinder: 'toWorld' transformation contains shear!");
        }
        const double ir = 1.0 / l0, il = 1.0 / l2;
        ppg_shape s{};
        s.type = PPG_SHAPE_CYLINDER;
        for (int i = 0; i < 3; ++i) {
            s.to_world[4 * i] = (float)(o2w[4 * i] * ir); s.to_world[4 * i + 1] = (float)(o2w[4 * i + 1] * ir);
            s.to_world[4 * i + 2] = (float)(o2w[4 * i + 2] * il); s.to_world[4 * i + 3] = (float)o2w[4 * i + 3];
        }
        s.radius = (float)l0; s.length = (float)l2;
        s.emitter = -1;
        s.flip_normals = flip ? 1 : 0;
        return s;
    }

    // <emitter type="point" | "spot" | "directional"> (point.cpp:57-69, spot.cpp:68-94, directional.cpp:55-73) → ppg_delta_emitter; the same
    // values, in the same arithmetic, as ppg_host/mitsuba_xml.py parse_delta_emitter
    ppg_delta_emitter makeDeltaEmitter(const XmlNode &e) const {
        const std::string t = e.get("type");
        auto ep = props(e);
        const XmlNode *tw = nullptr;
        for (auto &c : e.children) if (c.tag == "transform" && (!c.attr("name") || c.get("name") == "toWorld")) { tw = &c; break; }
        const Mat4 m = tw ? transform(*tw) : Mat4::identity();
        auto xyz = [&](const char *tag, const char *name, float v[3]) {
            for (auto &c : e.children)
                if (c.tag == tag && c.get("name") == name) {
                    const char *ax[3] = {"x", "y", "z"};
                    for (int a = 0; a < 3; ++a) v[a] = c.attr(ax[a]) ? (float)std::stod(sub(c.get(ax[a]))) : 0.0f;
                    return true;
                }
            return false;
        };
        if (ep.count("samplingWeight") && std::stod(ep["samplingWeight"]) != 1.0) throw std::runtime_error(t + " emitter: a samplingWeight other than 1 is not supported");
        ppg_delta_emitter d{};
        d.to_local[0] = d.to_local[4] = d.to_local[8] = 1.0f;
        if (t == "point") {
            d.type = PPG_EMITTER_POINT;
            const bool hasPos = xyz("point", "position", d.position);
            if (hasPos && tw) throw std::runtime_error("point emitter: only one of the parameters 'position' and 'toWorld' can be used");
            if (!hasPos) for (int a = 0; a < 3; ++a) d.position[a] = m.m[4 * a + 3];
            colour(e, "intensity", 1.0f, d.intensity);
            return d;
        }
        if (t == "spot") {
            d.type = PPG_EMITTER_SPOT;
            for (auto &c : e.children) if (c.get("name") == "texture" || c.tag == "texture") throw std::runtime_error("spot emitter: a projection 'texture' is not supported");
            const float rad = 3.14159265358979323846f / 180.0f;  // degToRad, util.h
            const float cutoffDeg = ep.count("cutoffAngle") ? (float)std::stod(ep["cutoffAngle"]) : 20.0f;
            const float beamDeg = ep.count("beamWidth") ? (float)std::stod(ep["beamWidth"]) : cutoffDeg * 3.0f / 4.0f;
            d.cutoff_angle = cutoffDeg * rad; d.beam_width = beamDeg * rad;
            if (d.cutoff_angle < d.beam_width) throw std::runtime_error("spot emitter: cutoffAngle must not be smaller than beamWidth");
            if (!(0 < d.beam_width && cutoffDeg < 90)) throw std::runtime_error("spot emitter: the angles must satisfy 0 < beamWidth <= cutoffAngle < 90 degrees");
            for (int a = 0; a < 3; ++a) d.position[a] = m.m[4 * a + 3];
            inverse3(m, d.to_local);
            colour(e, "intensity", 1.0f, d.intensity);
            return d;
        }
        d.type = PPG_EMITTER_DIRECTIONAL;
        float v[3];
        const bool hasDir = xyz("vector", "direction", v);
        if (hasDir && tw) throw std::runtime_error("directional emitter: only one of the parameters 'direction' and 'toWorld' can be used at a time");
        if (hasDir) {
            const float ln = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            if (!(ln > 0)) throw std::runtime_error("directional emitter: 'direction' is zero");
            for (int a = 0; a < 3; ++a) d.direction[a] = v[a] / ln;
        } else {
            if (hasScale(m)) throw std::runtime_error("directional emitter: scale factors in the emitter-to-world transformation are not allowed");
            for (int a = 0; a < 3; ++a) d.direction[a] = m.m[4 * a + 2];
        }
        colour(e, "irradiance", 1.0f, d.intensity);
        return d;
    }
    // inverse of the upper 3x3 by cofactors in double, rounded to float (ppg_host/mitsuba_xml.py inverse3: the same operations)
    static void inverse3(const Mat4 &m, float out[9]) {
        const double a = m.m[0], b = m.m[1], c = m.m[2], d = m.m[4], e = m.m[5], f = m.m[6], g = m.m[8], h = m.m[9], i = m.m[10];
        const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
        const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det, (f * g - d * i) / det, (a * i - c * g) / det,
                               (c * d - a * f) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
        for (int k = 0; k < 9; ++k) out[k] = (float)inv[k];
    }
    // focalLength "<x>mm" → diagonal field of view (PerspectiveCamera::configure, sensor.cpp:264-276), in the reference's float arithmetic
    static double focalLengthFov(std::string f) {
        if (f.size() >= 2 && f.compare(f.size() - 2, 2, "mm") == 0) f = f.substr(0, f.size() - 2);
        char *end = nullptr;
        const float value = (float)strtod(f.c_str(), &end);
        if (f.empty() || *end != '\0') throw std::runtime_error("could not parse the focal length '" + f + "' (must be of the form <x>mm, where <x> is a positive number)");
        const float a = std::atan(std::sqrt((float)(36 * 36 + 24 * 24)) / (2 * value));
        return (double)(float)(2 * 180 / 3.14159265358979323846 * a);
    }
    // Transform::hasScale (transform.h:76-90)
    static bool hasScale(const Mat4 &t) {
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) {
                float sum = 0;
                for (int k = 0; k < 3; ++k) sum += t.m[4 * i + k] * t.m[4 * j + k];
                if (i == j ? std::abs(sum - 1) > 1e-3f : std::abs(sum) > 1e-3f) return true;
            }
        return false;
    }
    static void makeCamera(ppg_camera &cam, const Mat4 &c2w, double fov, const std::string &axisIn, double nearC, double farC, int W, int H) {
        // sensor.cpp:239-264, 301-305; perspective.cpp:150-164 (m_sampleToCamera), inverted in closed form
        const double aspect = (double)W / H, PI = 3.14159265358979323846;
        std::string axis = axisIn;
        if (axis == "smaller") axis = aspect > 1 ? "y" : "x";
        else if (axis == "larger") axis = aspect > 1 ? "x" : "y";
        double xfov;
        if (axis == "x") xfov = fov;
        else if (axis == "y") xfov = 2 * std::atan(std::tan(0.5 * fov * PI / 180) * aspect) * 180 / PI;
        else if (axis == "diagonal") { double diag = 2 * std::tan(0.5 * fov * PI / 180), w = diag / std::sqrt(1 + 1 / (aspect * aspect)); xfov = 2 * std::atan(w * 0.5) * 180 / PI; }
        else throw std::runtime_error("fovAxis '" + axisIn + "' not supported");
        const double cot = 1 / std::tan(xfov / 2 * PI / 180);
        double inv[16] = {0};
        inv[0] = -2 / cot; inv[3] = 1 / cot;
        inv[5] = -2 / (aspect * cot); inv[7] = 1 / (aspect * cot);
        inv[11] = 1;
        inv[14] = -(farC - nearC) / (nearC * farC); inv[15] = 1 / nearC;
        for (int i = 0; i < 16; ++i) { cam.sample_to_camera[i] = (float)inv[i]; cam.camera_to_world[i] = c2w.m[i]; }
        cam.near_clip = (float)nearC; cam.far_clip = (float)farC; cam.width = W; cam.height = H;
    }
    static void defaults(ppg_material &m) {  // what ppg_host.bindings.Material.from_dict fills in
        for (int k = 0; k < 3; ++k) { m.specular[k] = 1.0f; m.k[k] = 1.0f; }
        m.alpha = 0.1f;
        const bool cond = m.type == PPG_BSDF_MIRROR || m.type == PPG_BSDF_CONDUCTOR || m.type == PPG_BSDF_ROUGHCONDUCTOR;
        for (int k = 0; k < 3; ++k) m.eta[k] = cond ? 0.0f : 1.5046f;
    }
    // MicrofacetDistribution(props), microfacet.h:99-145: the distribution's name (the name of its table, data/microfacet/<name>.dat; flag
    // set on m), alpha = alphaU, and in m_mfd the general entry of a BSDF that states alphaU / alphaV, phong or sampleVisible = false
    // (ppg_microfacet; the same rule as ppg_host.bindings.Microfacet).  Bitmaps on the roughness are not read by this loader.
    std::string microfacet(const XmlNode &e, std::map<std::string, std::string> &p, const std::string &t, ppg_material &m) const {
        std::string distr = p.count("distribution") ? p["distribution"] : "beckmann";
        std::transform(distr.begin(), distr.end(), distr.begin(), ::tolower);
        if (distr != "ggx" && distr != "beckmann" && distr != "phong" && distr != "as")
            throw std::runtime_error(t + ": Specified an invalid distribution \"" + distr + "\", must be \"beckmann\", \"ggx\", or \"phong\"/\"as\"!");
        if ((distr == "phong" || distr == "as") && t != "roughplastic" && t != "roughcoating")  // as ppg_host/mitsuba_xml.py: phong from a scene file on roughplastic only
            throw std::runtime_error(t + ": distribution '" + distr + "' is not supported by the scene loaders on this plug-in (ggx, beckmann; phong on roughplastic)");
        if (distr == "as") distr = "phong";
        for (auto &c : e.children)
            if ((c.tag == "texture" || c.tag == "ref") && c.attr("name") && (c.get("name") == "alpha" || c.get("name") == "alphaU" || c.get("name") == "alphaV"))
                throw std::runtime_error(t + ": a texture on '" + c.get("name") + "' is not supported by this loader");
        if (distr == "beckmann") m.flags |= PPG_MAT_BECKMANN;  // Mitsuba's default (microfacet.h:99)
        m_mfd = ppg_microfacet{};
        if (p.count("alpha")) {
            if (p.count("alphaU") || p.count("alphaV")) throw std::runtime_error(t + ": Microfacet model: please specify either 'alpha' or 'alphaU'/'alphaV'.");
            m.alpha = std::stof(p["alpha"]);
        } else if (p.count("alphaU") || p.count("alphaV")) {
            if (!p.count("alphaU") || !p.count("alphaV")) throw std::runtime_error(t + ": Microfacet model: both 'alphaU' and 'alphaV' must be specified.");
            m.alpha = std::stof(p["alphaU"]);
            m_mfd.general = 1;
            m_mfd.alpha_v = std::stof(p["alphaV"]);
        } else m.alpha = 0.1f;
        const bool sampleAll = p.count("sampleVisible") && !flag(p, "sampleVisible", true);
        if (distr == "phong" || sampleAll) {
            if (!m_mfd.general) m_mfd.alpha_v = m.alpha;
            m_mfd.general = 1;
            m_mfd.distribution = distr == "phong" ? 1 : 0;
            m_mfd.sample_all = sampleAll ? 1 : 0;
        }
        return distr;
    }
    double lookupIOR(const std::map<std::string, std::string> &p, const std::string &name, const std::string &dflt) const {  // ior.h:95-111
        static const std::map<std::string, double> ior = {{"vacuum", 1.0}, {"air", 1.000277}, {"water", 1.3330}, {"polypropylene", 1.49}, {"bk7", 1.5046}, {"diamond", 2.419}};
        std::string v = p.count(name) ? p.at(name) : dflt;
        char *end = nullptr;
        double d = std::strtod(v.c_str(), &end);
        if (end && *end == '\0' && end != v.c_str()) return d;
        std::transform(v.begin(), v.end(), v.begin(), ::tolower);
        auto it = ior.find(v);
        if (it == ior.end()) throw std::runtime_error("IOR name '" + v + "' is not in the built-in list; give a number");
        return it->second;
    }
    void conductorIOR(const XmlNode &e, const std::map<std::string, std::string> &p, const std::string &what, ppg_material &m) const {
        const float ext = (float)lookupIOR(p, "extEta", "air");
        std::string mat = p.count("material") ? p.at("material") : "Cu";
        std::transform(mat.begin(), mat.end(), mat.begin(), ::tolower);
        float eta[3] = {0, 0, 0}, k[3] = {1, 1, 1};
        if (mat != "none") {
            const std::string name = p.count("material") ? p.at("material") : "Cu";
            if (!hasChildNamed(e, "eta") || !hasChildNamed(e, "k")) {  // the measured spectra ship with Mitsuba (data/ior/<name>.{eta,k}.spd)
                std::string dir = m_dataDir;
                if (dir.empty()) { const char *ev = std::getenv("PPG_MITSUBA_DATA"); if (ev) dir = ev; }
                std::vector<double> le, ve, lk, vk;
                if (dir.empty() || !readSPD(dir + "/ior/" + name + ".eta.spd", le, ve) || !readSPD(dir + "/ior/" + name + ".k.spd", lk, vk) || le.size() < 2 || lk.size() < 2)
                    throw std::runtime_error(what + "(material=" + name + "): the measured IOR spectra data/ior/" + name + ".{eta,k}.spd come with Mitsuba: pass --data-dir / PPG_MITSUBA_DATA, or give eta and k");
                interpolatedToRGB(le, ve, eta, false, false);
                interpolatedToRGB(lk, vk, k, false, false);
            }
            if (hasChildNamed(e, "eta")) colour(e, "eta", 0.0f, eta);
            if (hasChildNamed(e, "k")) colour(e, "k", 1.0f, k);
        }
        for (int c = 0; c < 3; ++c) { m.eta[c] = eta[c] / ext; m.k[c] = k[c] / ext; }
    }
    // (the general microfacet entry of the BSDF it built last — at most one rough plug-in sits inside the adapters — is left in m_mfd, its
    // coating / roughcoating in m_coat)
    ppg_material makeBsdfTop(const XmlNode &e, LoadedScene &out) const { m_mfd = ppg_microfacet{}; m_coat = ppg_coating{}; m_blend = BlendSpec{}; return makeBsdf(e, true, out); }
    // The blended material's own record — diffuse, carrying nothing but the adapters that go around it — with the combinator left in m_blend
    // (the same rules as ppg_host/mitsuba_xml.py).  The nesting order this build knows is bumpmap(mask(twosided(blend(leaf, ..)))); a child is
    // a nested <bsdf> or a <ref> to a <bsdf> with an id that stands before it.
    ppg_material blended(const XmlNode &e, std::map<std::string, std::string> &p, const std::string &t, LoadedScene &out) const {
        std::vector<const XmlNode *> in;
        for (auto &c : e.children)  // (a <ref> to a texture is no child: as ppg_host/mitsuba_xml.py skips it)
            if (c.tag == "bsdf" || (c.tag == "ref" && c.get("name") != "weight" && !m_textureIds.count(c.get("id")))) in.push_back(&c);
        if (in.size() > PPG_BLEND_MAX) throw std::runtime_error(t + ": more than 4 nested bsdfs are not supported (found " + std::to_string(in.size()) + ")");
        if (t == "blendbsdf" && in.size() != 2)
            throw std::runtime_error("blendbsdf: BSDF count mismatch: expected two nested BSDF instances! (found " + std::to_string(in.size()) + ")");
        BlendSpec spec;
        for (const XmlNode *c : in) {
            ppg_material m{};
            ppg_microfacet g{};
            std::string it;
            bool isBlend = false, isCoated = false;
            if (c->tag == "ref") {
                auto f = m_byId.find(c->get("id"));
                if (f == m_byId.end()) throw std::runtime_error(t + ": <ref id=\"" + c->get("id") + "\">: no such bsdf before it");
                it = "ref " + c->get("id");
                m = out.scene.materials[f->second]; g = m_mfdOf[f->second];
                isBlend = m_blendOf[f->second].b.kind != 0; isCoated = m_coatOf[f->second].kind != 0;
            } else {
                it = c->get("type");
                if (it == "twosided" || it == "mask" || it == "bumpmap")
                    throw std::runtime_error(t + "(" + it + ") is not supported: the nesting order is bumpmap(mask(twosided(" + t + "(..))))");
                m_mfd = ppg_microfacet{}; m_coat = ppg_coating{}; m_blend = BlendSpec{};
                m = makeBsdf(*c, false, out);
                g = m_mfd;
                isBlend = m_blend.b.kind != 0; isCoated = m_coat.kind != 0;
            }
            m_mfd = ppg_microfacet{}; m_coat = ppg_coating{}; m_blend = BlendSpec{};
            if (isBlend) throw std::runtime_error(t + "(" + it + "): blends of blends are not supported");
            if (isCoated) throw std::runtime_error(t + "(" + it + "): coated children are not supported");
            if (m.type == PPG_BSDF_DIELECTRIC || m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_ROUGHDIELECTRIC)
                throw std::runtime_error(t + "(" + it + "): dielectric, thindielectric and roughdielectric children are not supported");
            if (m.type == PPG_BSDF_ROUGHDIFFUSE || m.type == PPG_BSDF_DIFFTRANS || m.type == PPG_BSDF_PHONG)
                throw std::runtime_error(t + "(" + it + "): roughdiffuse, difftrans and phong children are not supported");
            if (m.type == PPG_BSDF_TWOSIDED_DIFFUSE || (m.flags & (PPG_MAT_TWOSIDED | PPG_MAT_MASK)) || (m.texture >> 16))
                throw std::runtime_error(t + "(" + it + ") is not supported: the nesting order is bumpmap(mask(twosided(" + t + "(..))))");
            spec.kids.push_back(m);
            spec.kidMfd.push_back(g);
        }
        ppg_blend &b = spec.b;
        b.n = (uint32_t)in.size();
        if (t == "blendbsdf") {
            b.kind = 1;
            if (p.count("weight")) {
                char *end = nullptr;
                const std::string ws = p["weight"];
                b.weight[0] = (float)strtod(ws.c_str(), &end);
                if (ws.empty() || *end != '\0') throw std::runtime_error("blendbsdf: Could not parse the weight!");
            } else b.weight[0] = 0.5f;
            for (auto &c : e.children)
                if ((c.tag == "texture" || c.tag == "ref") && c.get("name") == "weight") {  // (this loader reads no bitmaps)
                    if (m_strict) throw std::runtime_error("blendbsdf: textured 'weight' is not supported (SURVEY.md §8 f1)");
                    m_lenientNotes.push_back("texture on 'weight' ignored: the plug-in's default value is used");
                    b.weight[0] = 0.5f;
                }
            if (!std::isfinite(b.weight[0]) || b.weight[0] < 0) throw std::runtime_error("blendbsdf: weight must be finite and not negative");
        } else {
            b.kind = 2;
            const std::string ws = p.count("weights") ? p["weights"] : "";
            std::vector<float> w;
            size_t pos = 0;
            while (pos < ws.size()) {  // tokenize(.., " ,;"), mixturebsdf.cpp:70-84
                const size_t a = ws.find_first_not_of(" ,;", pos);
                if (a == std::string::npos) break;
                size_t z = ws.find_first_of(" ,;", a);
                if (z == std::string::npos) z = ws.size();
                const std::string tok = ws.substr(a, z - a);
                char *end = nullptr;
                const double v = strtod(tok.c_str(), &end);
                if (*end != '\0') throw std::runtime_error("mixturebsdf: Could not parse the BSDF weights!");
                w.push_back((float)v);
                pos = z;
            }
            if (w.empty()) throw std::runtime_error("mixturebsdf: No weights were supplied!");
            if (w.size() != in.size())
                throw std::runtime_error("mixturebsdf: BSDF count mismatch: " + std::to_string(in.size()) + " bsdfs, but specified " + std::to_string(w.size()) + " weights");
            double sum = 0;
            for (size_t k = 0; k < w.size(); ++k) {
                if (!std::isfinite(w[k]) || w[k] < 0) throw std::runtime_error("mixturebsdf: weights must be finite and not negative");
                b.weight[k] = w[k];
                sum += w[k];
            }
            if (!(sum > 0)) throw std::runtime_error("mixturebsdf: The weights must sum to a value greater than zero!");
            b.ensure_energy_conservation = flag(p, "ensureEnergyConservation", true) ? 1 : 0;
        }
        m_blend = spec;
        ppg_material m{};
        m.type = PPG_BSDF_DIFFUSE; defaults(m);
        m.reflectance[0] = m.reflectance[1] = m.reflectance[2] = 0.5f;
        return m;
    }
    // The nested BSDF's record, with the adapter's parameters left in m_coat (ppg_coating; the same rules as ppg_host/mitsuba_xml.py).  The
    // nesting order this build knows is bumpmap(mask(twosided(coating(leaf)))); the plug-ins' parameters are constants.
    ppg_material coated(const XmlNode &e, std::map<std::string, std::string> &p, const std::string &t, const std::vector<const XmlNode *> &in, LoadedScene &out) const {
        if (in.size() != 1) throw std::runtime_error(t + ": exactly one nested bsdf is required (found " + std::to_string(in.size()) + ")");
        const std::string it = in[0]->get("type");
        if (it == "coating" || it == "roughcoating" || it == "twosided" || it == "mask" || it == "bumpmap")
            throw std::runtime_error(t + "(" + it + ") is not supported: the nesting order is bumpmap(mask(twosided(coating(..))))");
        if (it == "blendbsdf" || it == "mixturebsdf") throw std::runtime_error(t + "(" + it + ") is not supported: neither a coat around a blend nor a coated child");
        for (auto &c : e.children)
            if ((c.tag == "texture" || c.tag == "ref") && c.attr("name") &&
                (c.get("name") == "sigmaA" || c.get("name") == "specularReflectance" || c.get("name") == "alpha" || c.get("name") == "alphaU" || c.get("name") == "alphaV"))
                throw std::runtime_error(t + ": a texture on '" + c.get("name") + "' is not supported");
        ppg_material m = makeBsdf(*in[0], false, out);
        if (m.type == PPG_BSDF_DIELECTRIC || m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_ROUGHDIELECTRIC)
            throw std::runtime_error(t + "(" + it + "): a coat on dielectric, thindielectric or roughdielectric is not supported");
        if (m.type == PPG_BSDF_ROUGHDIFFUSE || m.type == PPG_BSDF_DIFFTRANS || m.type == PPG_BSDF_PHONG)
            throw std::runtime_error(t + "(" + it + "): a coat on roughdiffuse, difftrans or phong is not supported");
        if (t == "roughcoating" && (m.type == PPG_BSDF_MIRROR || m.type == PPG_BSDF_CONDUCTOR || m.type == PPG_BSDF_PLASTIC))
            throw std::runtime_error("roughcoating(" + it + "): a roughcoating over a BSDF with a delta component (conductor, plastic) is not supported");
        const double intIOR = lookupIOR(p, "intIOR", "bk7"), extIOR = lookupIOR(p, "extIOR", "air");
        if (intIOR < 0 || extIOR < 0 || intIOR == extIOR) throw std::runtime_error(t + ": The interior and exterior indices of refraction must be positive and differ!");
        ppg_coating c{};
        c.kind = t == "coating" ? 1 : 2;
        c.eta = (float)(intIOR / extIOR);
        c.thickness = p.count("thickness") ? std::stof(p["thickness"]) : 1.0f;
        colour(e, "sigmaA", 0.0f, c.sigma_a);
        colour(e, "specularReflectance", 1.0f, c.specular);
        if (!(c.eta > 0 && c.eta != 1.0f)) throw std::runtime_error(t + ": The interior and exterior indices of refraction must be positive and differ!");
        bool finite = std::isfinite(c.eta) && std::isfinite(c.thickness);
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(c.sigma_a[k]) && std::isfinite(c.specular[k]);
        if (!finite) throw std::runtime_error(t + ": a parameter is not finite");
        if (c.thickness < 0 || c.sigma_a[0] < 0 || c.sigma_a[1] < 0 || c.sigma_a[2] < 0) throw std::runtime_error(t + ": thickness and sigmaA must not be negative");
        if (c.kind == 2) {
            const ppg_microfacet nested = m_mfd;  // (microfacet() leaves the layer's own entry there)
            ppg_material tmp{};
            const std::string distr = microfacet(e, p, t, tmp);
            const ppg_microfacet own = m_mfd;
            m_mfd = nested;
            if (own.general && std::max(own.alpha_v, 1e-4f) != std::max(tmp.alpha, 1e-4f))  // roughcoating.cpp:143-145 (the plug-in's own words)
                throw std::runtime_error("roughcoating: The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!");
            if (!std::isfinite(tmp.alpha)) throw std::runtime_error("roughcoating: a parameter is not finite");
            c.alpha = tmp.alpha;
            c.distribution = distr == "beckmann" ? 0 : (distr == "ggx" ? 1 : 2);
            c.sample_all = own.general && own.sample_all ? 1 : 0;
            char key[96];  // the reduction roughplastic uses, interned with its slices
            snprintf(key, sizeof key, "%s/%.9g/%.9g", distr.c_str(), c.alpha, c.eta);
            auto f = m_rtIndex.find(key);
            if (f == m_rtIndex.end()) {
                std::vector<float> slice;
                try { slice = roughplasticSlice(distr, c.alpha, c.eta, m_dataDir); }
                catch (const std::exception &ex) { throw std::runtime_error(t + ": " + ex.what()); }
                out.scene.rtransSamples = (uint32_t)slice.size() - 1;
                f = m_rtIndex.emplace(key, (int)(out.scene.rtrans.size() / slice.size())).first;
                out.scene.rtrans.insert(out.scene.rtrans.end(), slice.begin(), slice.end());
            }
            c.rtrans = f->second;
        }
        m_coat = c;
        return m;
    }
    // roughdiffuse (roughdiffuse.cpp:88-122), difftrans (difftrans.cpp:49-74) and phong (phong.cpp:60-107) with Mitsuba's parameter names and
    // defaults, then BSDF::ensureEnergyConservation (bsdf.cpp:88-146) as their configure() calls it: the same rules and the same float
    // arithmetic as ppg_host/mitsuba_xml.py.  This loader reads no parameter bitmaps.
    ppg_material lobe(const XmlNode &e, std::map<std::string, std::string> &p, const std::string &t, LoadedScene &out) const {
        ppg_material m{};
        auto textured = [&](const std::string &name) {
            for (auto &c : e.children) if ((c.tag == "texture" || c.tag == "ref") && c.get("name") == name) return true;
            return false;
        };
        auto number = [&](const std::string &name, float dflt) {
            if (textured(name)) {
                if (m_strict) throw std::runtime_error(t + ": a texture on '" + name + "' is not supported (a bitmap on its reflectance is)");
                m_lenientNotes.push_back("texture on '" + name + "' ignored: the plug-in's default value is used");
                return dflt;
            }
            return p.count(name) ? std::stof(p[name]) : dflt;
        };
        float *pair[2] = {m.reflectance, nullptr};
        std::string names = "\"reflectance\"";
        if (t == "roughdiffuse") {
            m.type = PPG_BSDF_ROUGHDIFFUSE; defaults(m);
            m.alpha = number("alpha", 0.2f);
            colour(e, hasChildNamed(e, "reflectance") || !hasChildNamed(e, "diffuseReflectance") ? "reflectance" : "diffuseReflectance", 0.5f, m.reflectance);
            if (flag(p, "useFastApprox", false)) m.flags |= PPG_MAT_FAST_APPROX;
        } else if (t == "difftrans") {
            m.type = PPG_BSDF_DIFFTRANS; defaults(m);
            colour(e, hasChildNamed(e, "transmittance") || !hasChildNamed(e, "diffuseTransmittance") ? "transmittance" : "diffuseTransmittance", 0.5f, m.reflectance);
            names = "\"transmittance\"";
        } else {
            m.type = PPG_BSDF_PHONG; defaults(m);
            if (m_strict && textured("specularReflectance"))
                throw std::runtime_error("phong: a texture on 'specularReflectance' is not supported (a bitmap on its diffuseReflectance is)");
            m.alpha = number("exponent", 30.0f);
            colour(e, "specularReflectance", 0.2f, m.specular);
            colour(e, "diffuseReflectance", 0.5f, m.reflectance);
            pair[0] = m.specular; pair[1] = m.reflectance;
            names = "\"specularReflectance\" and \"diffuseReflectance\"";
        }
        if (flag(p, "ensureEnergyConservation", true)) {
            float actual = 0.0f;
            for (int k = 0; k < 3; ++k) actual = std::max(actual, 0.0f + pair[0][k] + (pair[1] ? pair[1][k] : 0.0f));
            if (actual > 1) {
                const float scale = 0.99f * (1.0f / actual);
                std::ostringstream w;
                w << "bsdf '" << t << "' violates energy conservation: " << names << (pair[1] ? " sum to" : " has") << " a component-wise maximum of " << actual
                  << " (> 1) and will be scaled by " << scale << " (ensureEnergyConservation=false prevents this)";
                out.warnings.push_back(w.str());
                for (int k = 0; k < 3; ++k) { pair[0][k] *= scale; if (pair[1]) pair[1][k] *= scale; }
            }
        }
        return m;
    }
    ppg_material makeBsdf(const XmlNode &e, bool allowWrap, LoadedScene &out) const {
        std::string t = e.get("type");
        auto p = props(e);
        ppg_material m{};
        auto inner = [&]() { std::vector<const XmlNode *> v; for (auto &c : e.children) if (c.tag == "bsdf") v.push_back(&c); return v; };
        if (t == "diffuse") { m.type = PPG_BSDF_DIFFUSE; defaults(m); colour(e, "reflectance", 0.5f, m.reflectance); return m; }
        if (t == "twosided" && allowWrap) {
            auto in = inner();
            if (in.size() == 1) {
                m = makeBsdf(*in[0], false, out);
                if (m.type == PPG_BSDF_DIELECTRIC || m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_ROUGHDIELECTRIC) throw std::runtime_error("twosided(dielectric): only BRDFs can be two-sided (twosided.cpp:84-88)");
                if (m.type == PPG_BSDF_DIFFTRANS) throw std::runtime_error("twosided(difftrans): only BRDFs can be two-sided (twosided.cpp:84-88)");
                if (m.type == PPG_BSDF_NULL) throw std::runtime_error("twosided(null): only BRDFs can be two-sided (twosided.cpp:84-88)");
                if (m.type == PPG_BSDF_DIFFUSE && !(m.flags & PPG_MAT_MASK) && !m_blend.b.kind) { m.type = PPG_BSDF_TWOSIDED_DIFFUSE; return m; }
                m.flags |= PPG_MAT_TWOSIDED;
                return m;
            }
            t = "twosided(...)";
        } else if (t == "mask" && allowWrap) {
            auto in = inner();
            if (in.size() == 1) {
                m = makeBsdf(*in[0], true, out);
                if (m.flags & PPG_MAT_MASK) throw std::runtime_error("mask(mask(...)) is not supported");
                if (m.type == PPG_BSDF_NULL) throw std::runtime_error("mask(null) is not supported");
                if (m.type == PPG_BSDF_TWOSIDED_DIFFUSE) { m.type = PPG_BSDF_DIFFUSE; m.flags |= PPG_MAT_TWOSIDED; }
                m.flags |= PPG_MAT_MASK;
                colour(e, "opacity", 0.5f, m.opacity);
                return m;
            }
            t = "mask(...)";
        } else if (t == "conductor") {
            std::string mat = p.count("material") ? p["material"] : "Cu";
            std::transform(mat.begin(), mat.end(), mat.begin(), ::tolower);
            m.type = mat == "none" ? PPG_BSDF_MIRROR : PPG_BSDF_CONDUCTOR;
            defaults(m);
            colour(e, "specularReflectance", 1.0f, m.reflectance);
            if (mat != "none") conductorIOR(e, p, t, m);
            return m;
        } else if (t == "roughconductor" || t == "roughdielectric") {
            if (t == "roughconductor") {
                m.type = PPG_BSDF_ROUGHCONDUCTOR; defaults(m);
                colour(e, "specularReflectance", 1.0f, m.reflectance);
                conductorIOR(e, p, t, m);
            } else {  // roughdielectric.cpp:183-211
                m.type = PPG_BSDF_ROUGHDIELECTRIC; defaults(m);
                colour(e, "specularReflectance", 1.0f, m.reflectance); colour(e, "specularTransmittance", 1.0f, m.specular);
                const double intIOR = lookupIOR(p, "intIOR", "bk7"), extIOR = lookupIOR(p, "extIOR", "air");
                if (intIOR < 0 || extIOR < 0 || intIOR == extIOR) throw std::runtime_error(t + ": the interior and exterior indices of refraction must be positive and differ");
                m.eta[0] = m.eta[1] = m.eta[2] = (float)(intIOR / extIOR);
            }
            microfacet(e, p, t, m);
            return m;
        } else if (t == "roughplastic") {  // roughplastic.cpp:197-227, 285-305
            m.type = PPG_BSDF_ROUGHPLASTIC; defaults(m);
            colour(e, "diffuseReflectance", 0.5f, m.reflectance); colour(e, "specularReflectance", 1.0f, m.specular);
            const double intIOR = lookupIOR(p, "intIOR", "polypropylene"), extIOR = lookupIOR(p, "extIOR", "air");
            if (intIOR < 0 || extIOR < 0 || intIOR == extIOR) throw std::runtime_error(t + ": the interior and exterior indices of refraction must be positive and differ");
            m.eta[0] = m.eta[1] = m.eta[2] = (float)(intIOR / extIOR);
            if (flag(p, "nonlinear", false)) m.flags |= PPG_MAT_NONLINEAR;
            const std::string distr = microfacet(e, p, t, m);
            if (m_mfd.general && std::max(m_mfd.alpha_v, 1e-4f) != std::max(m.alpha, 1e-4f))  // roughplastic.cpp:221-223
                throw std::runtime_error(t + ": The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!");
            char key[96];
            snprintf(key, sizeof key, "%s/%.9g/%.9g", distr.c_str(), m.alpha, m.eta[0]);
            auto it = m_rtIndex.find(key);
            if (it == m_rtIndex.end()) {
                std::vector<float> slice;
                try { slice = roughplasticSlice(distr, m.alpha, m.eta[0], m_dataDir); }
                catch (const std::exception &ex) { throw std::runtime_error(t + ": " + ex.what()); }
                out.scene.rtransSamples = (uint32_t)slice.size() - 1;
                it = m_rtIndex.emplace(key, (int)(out.scene.rtrans.size() / slice.size())).first;
                out.scene.rtrans.insert(out.scene.rtrans.end(), slice.begin(), slice.end());
            }
            m.rtrans = it->second;
            return m;
        } else if (t == "plastic" || t == "dielectric" || t == "thindielectric") {
            m.type = t == "plastic" ? PPG_BSDF_PLASTIC : (t == "dielectric" ? PPG_BSDF_DIELECTRIC : PPG_BSDF_THINDIELECTRIC);
            defaults(m);
            const float eta = (float)(lookupIOR(p, "intIOR", t == "plastic" ? "polypropylene" : "bk7") / lookupIOR(p, "extIOR", "air"));
            m.eta[0] = m.eta[1] = m.eta[2] = eta;
            if (t == "plastic") {
                colour(e, "diffuseReflectance", 0.5f, m.reflectance); colour(e, "specularReflectance", 1.0f, m.specular);
                if (flag(p, "nonlinear", false)) m.flags |= PPG_MAT_NONLINEAR;
            } else {
                colour(e, "specularReflectance", 1.0f, m.reflectance); colour(e, "specularTransmittance", 1.0f, m.specular);
            }
            return m;
        }
        if (t == "roughdiffuse" || t == "difftrans" || t == "phong") return lobe(e, p, t, out);
        if (t == "null") {  // null.cpp:36-80: no parameters (a coat on it, its use in a blend or on an analytic shape: ppg_set_scene refuses)
            m.type = PPG_BSDF_NULL; defaults(m);
            m.reflectance[0] = m.reflectance[1] = m.reflectance[2] = 1.0f;
            return m;
        }
        if (t == "coating" || t == "roughcoating") {  // SmoothCoating (coating.cpp:109-200), RoughCoating (roughcoating.cpp:114-227): the innermost adapter
            auto in = inner();
            try { return coated(e, p, t, in, out); }
            catch (const std::runtime_error &ex) {
                if (m_strict) throw;
                m_coat = ppg_coating{};
                if (in.size() == 1) {  // where a strict load refuses this coat, a lenient one renders the nested BSDF
                    out.warnings.push_back("bsdf '" + t + "' dropped around its nested bsdf (" + ex.what() + ")");
                    return makeBsdf(*in[0], allowWrap, out);
                }
            }
        }
        if (t == "blendbsdf" || t == "mixturebsdf") {  // BlendBSDF (blendbsdf.cpp:70-133), MixtureBSDF (mixturebsdf.cpp:64-172): where a leaf stands
            try { return blended(e, p, t, out); }
            catch (const std::runtime_error &ex) {
                if (m_strict) throw;
                m_mfd = ppg_microfacet{}; m_coat = ppg_coating{}; m_blend = BlendSpec{};
                out.warnings.push_back("bsdf '" + t + "' replaced by diffuse(0.5) (" + ex.what() + ")");
                m = ppg_material{}; m.type = PPG_BSDF_DIFFUSE; defaults(m);
                m.reflectance[0] = m.reflectance[1] = m.reflectance[2] = 0.5f;
                return m;
            }
        }
        if (!m_strict && (t == "bumpmap" || t == "normalmap")) {  // adapters around one nested BSDF: render the nested one
            auto in = inner();
            if (in.size() == 1) { out.warnings.push_back("bsdf '" + t + "' dropped around its nested bsdf"); return makeBsdf(*in[0], allowWrap, out); }
        }
        if (m_strict) throw std::runtime_error("bsdf type '" + t + "' is not supported yet (diffuse, roughdiffuse, difftrans, phong, conductor, roughconductor, plastic, roughplastic, dielectric, thindielectric, roughdielectric, null, mask, twosided; SURVEY.md §8 f1)");
        out.warnings.push_back("bsdf '" + t + "' replaced by diffuse(0.5)");
        m = ppg_material{}; m.type = PPG_BSDF_DIFFUSE; defaults(m);
        m.reflectance[0] = m.reflectance[1] = m.reflectance[2] = 0.5f;
        return m;
    }
public:
    // The <bsdf> element carrying `id` (at any nesting depth: every element with an id is a named object in Mitsuba) as a ppg_material;
    // rough-transmittance slices it needs are appended to out.scene.rtrans.  Used by the Mitsuba plug-in shim
    // (mitsuba_plugin/guided_path_hip.cpp), which cannot reach the nested BSDF of an adapter through Mitsuba's API.
    bool bsdfById(const std::string &id, LoadedScene &out, ppg_material &m, ppg_microfacet *g = nullptr, ppg_coating *k = nullptr, BlendSpec *bl = nullptr) {
        std::ifstream f(m_path, std::ios::binary);
        if (!f) throw std::runtime_error("cannot open '" + m_path + "'");
        std::stringstream ss; ss << f.rdbuf();
        const std::string text = ss.str();
        XmlNode root = XmlParser(text).parseDocument();
        size_t slash = m_path.find_last_of('/');
        m_base = slash == std::string::npos ? "." : m_path.substr(0, slash);
        collectDefaults(root);
        for (auto &c : root.children) if (c.tag == "texture" && c.attr("id")) m_textureIds.insert(c.get("id"));
        const XmlNode *found = nullptr;
        std::function<void(const XmlNode &)> walk = [&](const XmlNode &n) {
            for (auto &c : n.children) {
                if (!found && c.tag == "bsdf" && c.attr("id") && c.get("id") == id) found = &c;
                if (!found) walk(c);
            }
        };
        walk(root);
        if (!found) return false;
        m = makeBsdfTop(*found, out);
        if (g) *g = m_mfd;
        else if (m_mfd.general) throw std::runtime_error("bsdf '" + id + "': alphaU / alphaV, distribution = phong and sampleVisible = false are not carried through this interface");
        if (k) *k = m_coat;
        else if (m_coat.kind) throw std::runtime_error("bsdf '" + id + "': coating / roughcoating are not carried through this interface");
        if (bl) *bl = m_blend;
        else if (m_blend.b.kind) throw std::runtime_error("bsdf '" + id + "': blendbsdf / mixturebsdf are not carried through this interface");
        return true;
    }
    // The ppg_material of a <bsdf> element that is not in a file: the plug-in shim builds one from a flat plug-in's Properties (a BSDF
    // without an id cannot be looked up in the scene file) and gets exactly what the scene loader makes of the same parameters.
    ppg_material bsdfFromElement(const XmlNode &e, LoadedScene &out, ppg_microfacet *g = nullptr, ppg_coating *k = nullptr) {
        m_base = ".";
        const ppg_material m = makeBsdfTop(e, out);
        if (g) *g = m_mfd;
        else if (m_mfd.general) throw std::runtime_error("alphaU / alphaV, distribution = phong and sampleVisible = false are not carried through this interface");
        if (k) *k = m_coat;
        else if (m_coat.kind) throw std::runtime_error("coating / roughcoating are not carried through this interface");
        if (m_blend.b.kind) throw std::runtime_error("blendbsdf / mixturebsdf are not carried through this interface");
        return m;
    }
private:
    // EAnisotropic of the material's BSDF: alphaU != alphaV (this loader reads no bitmaps on them); of a blended material: of any child
    bool anisotropic(uint32_t mat, const LoadedScene &out) const {
        const BlendSpec &bl = m_blendOf[mat];
        for (size_t k = 0; k < bl.kids.size(); ++k)
            if (bl.kidMfd[k].general && std::max(bl.kidMfd[k].alpha_v, 1e-4f) != std::max(bl.kids[k].alpha, 1e-4f)) return true;
        return m_mfdOf[mat].general && std::max(m_mfdOf[mat].alpha_v, 1e-4f) != std::max(out.scene.materials[mat].alpha, 1e-4f);
    }
    uint32_t intern(const ppg_material &m, LoadedScene &out, const ppg_microfacet &g = ppg_microfacet{}, const ppg_coating &coat = ppg_coating{},
                    const BlendSpec &blend = BlendSpec{}) {
        std::string key((const char *)&m, sizeof m);
        key.append((const char *)&g, sizeof g);
        key.append((const char *)&coat, sizeof coat);
        key.append((const char *)&blend.b, sizeof blend.b);
        for (const ppg_material &c : blend.kids) key.append((const char *)&c, sizeof c);
        for (const ppg_microfacet &c : blend.kidMfd) key.append((const char *)&c, sizeof c);
        for (size_t i = 0; i < m_matKeys.size(); ++i) if (m_matKeys[i] == key) return (uint32_t)i;
        m_matKeys.push_back(key);
        out.scene.materials.push_back(m);
        m_mfdOf.push_back(g);
        m_coatOf.push_back(coat);
        m_blendOf.push_back(blend);
        return (uint32_t)m_matKeys.size() - 1;
    }
};

namespace xml {
// one <bsdf id="..."> of a scene file as a ppg_material appended to `data` (its rough-transmittance slice, if any, to data.rtrans)
// (name, tag, value) triples of a flat BSDF plug-in's parameters → its ppg_material, through the scene loader's own <bsdf> handling:
// tag = float | integer | boolean | string | rgb, value as it would stand in the scene file ("0.1, 0.2, 0.3" for rgb)
struct BsdfParam { std::string name, tag, value; };
// g: receives the BSDF's general microfacet entry (ppg_set_microfacet; all zero: none); without it such a BSDF is refused
inline bool bsdfFromProperties(const std::string &plugin, const std::vector<BsdfParam> &params, const std::string &dataDir, SceneData &data, ppg_material &m, std::string &why,
                               ppg_microfacet *g = nullptr);
// (a coating / roughcoating is an adapter and has an id or a parent with one: it comes through bsdfById, k receiving its ppg_coating with
// rtrans already moved to the row of data.rtrans)

inline bool bsdfById(const std::string &scenePath, const std::string &id, const std::string &dataDir, SceneData &data, ppg_material &m, std::string &why,
                     ppg_microfacet *g = nullptr, ppg_coating *k = nullptr, BlendSpec *bl = nullptr) {
    try {
        SceneXmlLoader loader(scenePath, {}, true, 0, 0, dataDir);
        LoadedScene tmp;
        if (!loader.bsdfById(id, tmp, m, g, k, bl)) return false;
        if (!tmp.scene.rtrans.empty()) {
            if (data.rtransSamples && data.rtransSamples != tmp.scene.rtransSamples) { why = "rough-transmittance tables of different resolutions"; return false; }
            const uint32_t have = data.rtransSamples ? (uint32_t)(data.rtrans.size() / (data.rtransSamples + 1)) : 0u;
            data.rtransSamples = tmp.scene.rtransSamples;
            data.rtrans.insert(data.rtrans.end(), tmp.scene.rtrans.begin(), tmp.scene.rtrans.end());
            if (m.type == PPG_BSDF_ROUGHPLASTIC) m.rtrans += (int32_t)have;
            if (k && k->kind == 2) k->rtrans += (int32_t)have;
            if (bl) for (ppg_material &c : bl->kids) if (c.type == PPG_BSDF_ROUGHPLASTIC) c.rtrans += (int32_t)have;
        }
        return true;
    } catch (const std::exception &e) {
        why = e.what();
        return false;
    }
}

inline bool bsdfFromProperties(const std::string &plugin, const std::vector<BsdfParam> &params, const std::string &dataDir, SceneData &data, ppg_material &m, std::string &why,
                               ppg_microfacet *g) {
    try {
        SceneXmlLoader loader("", {}, true, 0, 0, dataDir);
        LoadedScene tmp;
        XmlNode e;
        e.tag = "bsdf"; e.attrs.push_back({"type", plugin});
        for (const BsdfParam &p : params) {
            XmlNode c;
            c.tag = p.tag; c.attrs.push_back({"name", p.name}); c.attrs.push_back({"value", p.value});
            e.children.push_back(c);
        }
        m = loader.bsdfFromElement(e, tmp, g);
        if (!tmp.scene.rtrans.empty()) {
            if (data.rtransSamples && data.rtransSamples != tmp.scene.rtransSamples) { why = "rough-transmittance tables of different resolutions"; return false; }
            const uint32_t have = data.rtransSamples ? (uint32_t)(data.rtrans.size() / (data.rtransSamples + 1)) : 0u;
            data.rtransSamples = tmp.scene.rtransSamples;
            data.rtrans.insert(data.rtrans.end(), tmp.scene.rtrans.begin(), tmp.scene.rtrans.end());
            if (m.type == PPG_BSDF_ROUGHPLASTIC) m.rtrans += (int32_t)have;
        }
        return true;
    } catch (const std::exception &e) {
        why = e.what();
        return false;
    }
}
}  // namespace xml

}  // namespace ppg
