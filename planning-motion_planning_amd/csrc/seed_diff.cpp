// seed_diff.cpp -- see seed_diff.hpp.  Host only.
#include "seed_diff.hpp"

#include <algorithm>

namespace eik {

namespace {

// the list sorted by (y, x, t0) with the first -- the lowest t0 -- of every cell kept
std::vector<SeedCell> per_cell_min(const SeedCell* s, int64_t n) {
    std::vector<SeedCell> v(s, s + (n > 0 ? n : 0));
    std::sort(v.begin(), v.end(), [](const SeedCell& a, const SeedCell& b) {
        if (a.y != b.y) return a.y < b.y;
        if (a.x != b.x) return a.x < b.x;
        return a.t0 < b.t0;
    });
    v.erase(std::unique(v.begin(), v.end(), [](const SeedCell& a, const SeedCell& b) { return a.x == b.x && a.y == b.y; }),
            v.end());
    return v;
}

bool before(const SeedCell& a, const SeedCell& b) { return a.y != b.y ? a.y < b.y : a.x < b.x; }

}  // namespace

SeedDiff seed_diff(const SeedCell* old_list, int64_t n_old, const SeedCell* new_list, int64_t n_new,
                   std::vector<RootDesc>& out) {
    const std::vector<SeedCell> o = per_cell_min(old_list, n_old), w = per_cell_min(new_list, n_new);
    SeedDiff d;
    out.clear();
    out.reserve(o.size());
    size_t j = 0;
    for (const SeedCell& c : o) {
        for (; j < w.size() && before(w[j], c); ++j) d.same = false;  // a new cell
        const bool hit = j < w.size() && w[j].x == c.x && w[j].y == c.y;
        const bool keep = hit && w[j].t0 <= c.t0;
        if (!hit || w[j].t0 != c.t0) d.same = false;
        if (hit) ++j;
        if (!keep) ++d.released;
        out.push_back(RootDesc{c.x, c.y, keep ? kRootKeep : kRootRelease, 0u, c.t0});
    }
    if (j < w.size()) d.same = false;
    return d;
}

}  // namespace eik
