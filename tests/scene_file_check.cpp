// Host-only check of host/scene_file.h — the .ppgs container — compiled with the address and undefined-behaviour sanitizers and run by
// tests/test_scene_file.py on the file that carries all fourteen optional blocks.  No device, no library: the header alone.
//   1. the file is read and written again: the same bytes;
//   2. every proper prefix of it is refused;
//   3. with the count of each counted block (spheres, delta emitters, shapes) set to 0x7fffffff it is refused, nothing sized by the claim;
//   4. with bit 14 set in the header's block word it is refused.
#include <cstdio>
#include <sstream>
#include <string>

#include "scene_file.h"

using namespace ppg;

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 40) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

bool loads(const std::string &bytes, SceneData &s) {
    std::istringstream f(bytes, std::ios::binary);
    try { return scene_file::load(f, s); } catch (const std::exception &) { return false; }
}
bool loads(const std::string &bytes) { SceneData s; return loads(bytes, s); }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { printf("usage: scene_file_check file.ppgs\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::stringstream whole; whole << in.rdbuf();
    const std::string a = whole.str();
    SceneData scene;
    CHECK(loadScene(argv[1], scene), "the file itself is refused");
    uint32_t flags = 0;
    if (a.size() >= 28) memcpy(&flags, &a[24], 4);
    CHECK(flags == (1u << scene_file::N_BITS) - 1, "the file carries blocks 0x%x, not all fourteen", flags);

    std::ostringstream again(std::ios::binary);
    CHECK(scene_file::save(again, scene), "save");
    CHECK(again.str() == a, "rewritten: %zu bytes, read %zu", again.str().size(), a.size());
    if (again.str() == a) printf("rewritten: %zu bytes, identical\n", a.size());

    size_t refused = 0;
    for (size_t n = 0; n < a.size(); ++n) {
        const bool ok = loads(a.substr(0, n));
        CHECK(!ok, "the prefix of %zu bytes is accepted", n);
        refused += !ok;
    }
    printf("prefixes refused: %zu of %zu\n", refused, a.size());

    // where each block starts: behind the fixed part, in the table's order, each as long as the writer makes it
    size_t at = 28 + scene.positions.size() * 4 + scene.normals.size() * 4 + scene.indices.size() * 4 + scene.triMaterial.size() * 8 +
                scene.materials.size() * sizeof(ppg_material) + scene.emitters.size() * sizeof(ppg_emitter) + sizeof(ppg_camera);
    int counted = 0, countedRefused = 0;
    for (const scene_file::Block &b : scene_file::blocks()) {
        if (!(flags & b.bit)) continue;
        std::ostringstream one(std::ios::binary);
        scene_file::Writer w{one};
        b.write(w, scene);
        if (b.bit == scene_file::SPHERES || b.bit == scene_file::DELTA_EMITTERS || b.bit == scene_file::SHAPES) {
            std::string bad = a;
            const uint32_t huge = 0x7fffffffu;
            uint32_t was = 0;
            memcpy(&was, &bad[at], 4);
            CHECK(was >= 1 && was <= 3, "block 0x%x: no count at offset %zu (%u)", b.bit, at, was);
            memcpy(&bad[at], &huge, 4);
            const bool ok = loads(bad);
            CHECK(!ok, "block 0x%x with a count of 0x7fffffff is accepted", b.bit);
            ++counted; countedRefused += !ok;
        }
        at += one.str().size();
    }
    CHECK(at == a.size(), "the blocks end at %zu, the file at %zu", at, a.size());
    printf("huge counts refused: %d of %d\n", countedRefused, counted);

    std::string unknown = a;
    const uint32_t more = flags | (1u << scene_file::N_BITS);
    memcpy(&unknown[24], &more, 4);
    CHECK(!loads(unknown), "a file with bit 14 set is accepted");
    if (!loads(unknown)) printf("unknown block refused\n");

    if (failures) { printf("%d check(s) FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
