// cost_diff_main.cpp -- diff_rects (cost_diff_rects.cpp) in a stand-alone program for the sanitizer build
// (`make san_cdiff`): seeded lists of changed tiles against a brute-force restatement of the rule.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cost_diff_rects.hpp"

using namespace eik;

namespace {

int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);      \
            ++fails;                                                    \
        }                                                               \
    } while (0)

// the rule on a dense grid of blocks, no map: the reference of one block side
std::vector<DiffRect> brute(const std::vector<DiffRecord>& list, int ntx, int nty, int side) {
    const int bx = (ntx + side - 1) / side, by = (nty + side - 1) / side;
    std::vector<DiffRect> grid((size_t)bx * by, DiffRect{0, 0, 0, 0, -1});
    for (const DiffRecord& r : list) {
        DiffRect& b = grid[(size_t)(r.tile / ntx / side) * bx + r.tile % ntx / side];
        const int kind = r.raised ? 0 : 1;
        if (b.kind < 0) {
            b = DiffRect{r.x0, r.y0, r.x1, r.y1, kind};
        } else {
            if (r.x0 < b.x0) b.x0 = r.x0;
            if (r.y0 < b.y0) b.y0 = r.y0;
            if (r.x1 > b.x1) b.x1 = r.x1;
            if (r.y1 > b.y1) b.y1 = r.y1;
            if (kind < b.kind) b.kind = kind;
        }
    }
    std::vector<DiffRect> out;
    for (const DiffRect& b : grid)
        if (b.kind >= 0) out.push_back(b);
    return out;
}

void one(std::mt19937_64& rng, int ntx, int nty, double share, int64_t cap) {
    std::vector<DiffRecord> list;
    std::uniform_real_distribution<double> u(0, 1);
    for (int t = 0; t < ntx * nty; ++t) {
        if (u(rng) >= share) continue;
        const int x = t % ntx * 64, y = t / ntx * 64;
        const int a = (int)(u(rng) * 64), b = (int)(u(rng) * 64), c = (int)(u(rng) * 64), d = (int)(u(rng) * 64);
        DiffRecord r{};
        r.x0 = x + (a < b ? a : b);
        r.x1 = x + (a < b ? b : a) + 1;
        r.y0 = y + (c < d ? c : d);
        r.y1 = y + (c < d ? d : c) + 1;
        r.changed = 1 + (uint32_t)(u(rng) * 100);
        r.raised = u(rng) < 0.3 ? 1 : 0;
        r.tile = t;
        list.push_back(r);
    }
    std::vector<DiffRect> out;
    const int side = diff_rects(list.data(), (int64_t)list.size(), ntx, cap, out);
    if (list.empty()) {
        CHECK(side == 0 && out.empty());
        return;
    }
    CHECK(side >= 1 && (side & (side - 1)) == 0);
    CHECK((int64_t)out.size() <= cap);
    if (side > 1) CHECK((int64_t)brute(list, ntx, nty, side / 2).size() > cap);
    const std::vector<DiffRect> want = brute(list, ntx, nty, side);
    CHECK(want.size() == out.size());
    for (size_t k = 0; k < out.size() && k < want.size(); ++k)
        CHECK(out[k].x0 == want[k].x0 && out[k].y0 == want[k].y0 && out[k].x1 == want[k].x1 && out[k].y1 == want[k].y1 &&
              out[k].kind == want[k].kind);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    const int shapes[][2] = {{1, 1}, {3, 3}, {4, 1}, {1, 4}, {33, 32}, {7, 5}, {64, 64}};
    for (const auto& s : shapes)
        for (double share : {0.0, 0.02, 0.3, 1.0})
            for (int64_t cap : {1, 2, 5, 1024}) one(rng, s[0], s[1], share, cap);
    std::vector<DiffRect> out(3);
    CHECK(diff_rects(nullptr, 0, 4, 8, out) == 0 && out.empty());
    if (fails) {
        std::printf("cost_diff_san: %d checks failed\n", fails);
        return 1;
    }
    std::printf("cost_diff_san: ok\n");
    return 0;
}
