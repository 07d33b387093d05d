// cost_diff_rects.cpp -- from the changed tiles' records to rectangles and kinds (cost_diff_rects.hpp).
#include "cost_diff_rects.hpp"

#include <algorithm>

namespace eik {

namespace {
struct Block {
    int by, bx;  // block row / column at the current side
    DiffRect r;
};
}  // namespace

// Level by level: the blocks of side 2s are merged from those of side s through a dense grid of slots
// (O(blocks + grid cells) per level, the grid shrinking by four), so 65536 changed tiles cost a fraction
// of a millisecond; only the final <= cap blocks are sorted.
int diff_rects(const DiffRecord* list, int64_t n, int ntx, int64_t cap, std::vector<DiffRect>& out) {
    out.clear();
    if (n <= 0 || ntx < 1 || cap < 1) return 0;
    std::vector<Block> cur, next;
    cur.reserve((size_t)n);
    int nty = 1;
    for (int64_t i = 0; i < n; ++i) {
        const DiffRecord& r = list[i];
        if (r.changed == 0 || r.tile < 0) continue;
        const int ty = r.tile / ntx, tx = r.tile % ntx;
        nty = std::max(nty, ty + 1);
        cur.push_back(Block{ty, tx, DiffRect{r.x0, r.y0, r.x1, r.y1, r.raised ? 0 : 1}});
    }
    if (cur.empty()) return 0;
    std::vector<int32_t> slot;
    for (int side = 1, div = 1;; side *= 2, div = 2) {
        // blocks of `side` tiles from the previous level's (div = 1: the tiles themselves, merging doubles)
        const int64_t nbx = (ntx + side - 1) / side, nby = (nty + side - 1) / side;
        slot.assign((size_t)(nbx * nby), -1);
        next.clear();
        for (const Block& b : cur) {
            const int by = b.by / div, bx = b.bx / div;
            int32_t& s = slot[(size_t)(by * nbx + bx)];
            if (s < 0) {
                s = (int32_t)next.size();
                next.push_back(Block{by, bx, b.r});
            } else {
                DiffRect& m = next[(size_t)s].r;
                m.x0 = std::min(m.x0, b.r.x0);
                m.y0 = std::min(m.y0, b.r.y0);
                m.x1 = std::max(m.x1, b.r.x1);
                m.y1 = std::max(m.y1, b.r.y1);
                m.kind = std::min(m.kind, b.r.kind);  // ANY wins
            }
        }
        cur.swap(next);
        // (one block is left at the latest when side covers the grid: cap >= 1 ends the loop)
        if ((int64_t)cur.size() <= cap || (nbx == 1 && nby == 1)) {
            std::sort(cur.begin(), cur.end(), [](const Block& a, const Block& b) { return a.by != b.by ? a.by < b.by : a.bx < b.bx; });
            out.reserve(cur.size());
            for (const Block& b : cur) out.push_back(b.r);
            return side;
        }
    }
}

}  // namespace eik
