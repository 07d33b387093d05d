// cost_diff_rects.hpp -- the tile records of the device cost diff (cost_diff.hip) and the
// host's rule from records to the rectangles and kinds of eik_fim2d_update.  Host only, no HIP:
// cost_diff_main.cpp runs it under the sanitizers (`make san_cdiff`).
#pragma once
#include <cstdint>
#include <vector>

namespace eik {

// One solver tile (kTile x kTile cells) of the diff, 32 bytes.  The box holds the changed cells, in raster
// coordinates, half-open; changed == 0: an unchanged tile (the box is 0, 0, 0, 0).
struct DiffRecord {
    int32_t x0, y0, x1, y1;
    uint32_t changed;  // cells with old != new as values (+0 == -0, +inf == +inf), or an invalid new
    uint32_t raised;   // cells with new > old
    uint32_t invalid;  // cells whose new is NaN or < 0 (counted as changed too)
    int32_t tile;      // ty * ntx + tx
};
// the compacted list's first 32 bytes
struct DiffHeader {
    uint64_t changed, raised, invalid;  // cells
    uint64_t tiles;                     // changed tiles = list entries behind the header
};
static_assert(sizeof(DiffRecord) == 32 && sizeof(DiffHeader) == 32, "one header per record slot");

struct DiffRect {
    int64_t x0, y0, x1, y1;
    int kind;  // EIK_CHANGE_ANY (0) when a member tile has a raised cell, else EIK_CHANGE_LOWERED (1)
};

// The rule.  A changed tile's rectangle is its box, ANY if it holds a raised cell, else LOWERED.  More than
// cap of them: the union per block of 2 x 2 tiles (aligned to the tile grid's origin; the members' bounding
// box, ANY if any member is), then 4 x 4, 8 x 8, ... until at most cap are left.  Emitted in ascending
// (block row, block column).  list: n changed-tile records in any order, tiles of an ntx-wide grid;
// cap >= 1.  Returns the block side in tiles (1, 2, 4, ...), 0 when n == 0.
int diff_rects(const DiffRecord* list, int64_t n, int ntx, int64_t cap, std::vector<DiffRect>& out);

}  // namespace eik
