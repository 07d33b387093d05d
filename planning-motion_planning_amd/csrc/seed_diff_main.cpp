// seed_diff_main.cpp -- stand-alone driver of seed_diff.cpp for the host sanitizer build
// (`make -C csrc san_diff`: ASan + UBSan, no HIP, no GPU).  Checks the diff against a quadratic
// restatement of the rule on crafted and random lists; exit status 0 = all cases agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "seed_diff.hpp"

using namespace eik;

static double cell_min(const std::vector<SeedCell>& v, int x, int y) {
    double b = std::numeric_limits<double>::infinity();
    for (const SeedCell& s : v)
        if (s.x == x && s.y == y && s.t0 < b) b = s.t0;
    return b;
}

static int check(const char* name, const std::vector<SeedCell>& o, const std::vector<SeedCell>& w) {
    std::vector<RootDesc> out;
    const SeedDiff d = seed_diff(o.data(), (int64_t)o.size(), w.data(), (int64_t)w.size(), out);
    int bad = 0;
    int64_t released = 0;
    bool same = true;
    // every old cell exactly once, with its minimum and the class of the rule
    for (const SeedCell& s : o) {
        int hits = 0;
        for (const RootDesc& r : out)
            if (r.x == s.x && r.y == s.y) {
                ++hits;
                const double bo = cell_min(o, s.x, s.y), bn = cell_min(w, s.x, s.y);
                if (r.b_old != bo || r.cls != (bn <= bo ? kRootKeep : kRootRelease) || r.lifted != 0u) ++bad;
            }
        if (hits != 1) ++bad;
    }
    for (size_t i = 0; i < out.size(); ++i) {
        if (cell_min(o, out[i].x, out[i].y) == std::numeric_limits<double>::infinity()) ++bad;  // not an old cell
        if (i && !(out[i - 1].y < out[i].y || (out[i - 1].y == out[i].y && out[i - 1].x < out[i].x))) ++bad;
        released += out[i].cls == kRootRelease;
        if (cell_min(w, out[i].x, out[i].y) != out[i].b_old) same = false;
    }
    for (const SeedCell& s : w)
        if (cell_min(o, s.x, s.y) == std::numeric_limits<double>::infinity()) same = false;
    if (released != d.released || same != d.same) ++bad;
    std::printf("%-28s old %3zu new %3zu entries %3zu released %3ld same %d  %s\n", name, o.size(), w.size(), out.size(),
                (long)d.released, (int)d.same, bad ? "FAIL" : "ok");
    return bad;
}

int main() {
    int bad = 0;
    const std::vector<SeedCell> five = {{20, 20, 0.0}, {150, 30, 5.0}, {150, 160, 12.5}, {64, 64, 3.0}, {63, 64, 40.0}};
    bad += check("identical", five, five);
    bad += check("K = 1", {{3, 4, 0.0}}, {{3, 4, 0.0}});
    bad += check("K = 1 raised", {{3, 4, 0.0}}, {{3, 4, 1.0}});
    bad += check("K = 1 moved", {{3, 4, 0.0}}, {{4, 3, 0.0}});
    bad += check("disjoint", five, {{1, 1, 0.0}, {2, 2, 7.0}});
    bad += check("duplicates on a cell", {{5, 5, 2.0}, {5, 5, 1.0}, {9, 9, 0.0}}, {{5, 5, 2.0}, {9, 9, 0.0}});
    bad += check("duplicate dropped, same min", {{5, 5, 2.0}, {5, 5, 1.0}}, {{5, 5, 1.0}});
    bad += check("lowered and added", five, {{20, 20, 0.0}, {150, 30, 2.0}, {150, 160, 12.5}, {64, 64, 3.0}, {63, 64, 40.0}, {7, 7, 1.0}});
    bad += check("empty new list", five, {});
    bad += check("empty old list", {}, five);
    // random lists on a small raster: many shared cells
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&s]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    };
    for (int it = 0; it < 200; ++it) {
        std::vector<SeedCell> o(rnd() % 40), w(rnd() % 40);
        for (SeedCell& c : o) c = SeedCell{(int32_t)(rnd() % 6), (int32_t)(rnd() % 6), (double)(rnd() % 4)};
        for (SeedCell& c : w) c = SeedCell{(int32_t)(rnd() % 6), (int32_t)(rnd() % 6), (double)(rnd() % 4)};
        char name[32];
        std::snprintf(name, sizeof name, "random %d", it);
        bad += check(name, o, w);
    }
    std::printf("%s\n", bad ? "seed_diff: FAILED" : "seed_diff: all cases agree");
    return bad ? 1 : 0;
}
