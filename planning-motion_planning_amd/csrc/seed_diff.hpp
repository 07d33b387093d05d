// seed_diff.hpp -- the host's diff of two seed lists for the seeded re-solve (replan.hip, DESIGN.md
// §3.14).  Host only, no HIP: the sanitizer build (`make san`) and seed_diff_main.cpp cover it.
#pragma once
#include <cstdint>
#include <vector>

namespace eik {

constexpr int kRootKeep = 0, kRootRelease = 1;
// One entry per distinct cell of the OLD list.  b_old: the smallest t0 of the old seeds on the cell
// (t0 already rounded to the solve's dtype).  cls: keep when b_new <= b_old, release when b_new > b_old
// (no new seed on the cell: b_new = +inf).  lifted: written by the device (replan_roots_kernel).
struct RootDesc {
    int32_t x, y;
    int32_t cls;
    uint32_t lifted;
    double b_old;
};

struct SeedCell {
    int32_t x, y;
    double t0;  // finite, >= 0, never -0 or NaN: values order like their bit patterns
};

struct SeedDiff {
    int64_t released = 0;  // entries of class release
    bool same = true;      // b_new == b_old on every cell: the edit changes nothing
};

// O((n_old + n_new) log): both lists sorted by cell and reduced to their per-cell minimum, then one
// merge.  out: the entries, ordered by (y, x).
SeedDiff seed_diff(const SeedCell* old_list, int64_t n_old, const SeedCell* new_list, int64_t n_new,
                   std::vector<RootDesc>& out);

}  // namespace eik
