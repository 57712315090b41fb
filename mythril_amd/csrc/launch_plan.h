// Planner of the interpreter's direct launches (capi.cpp: mh_run_async, mh_repair_score,
// eval_values_rows): a tape set's ids bucketed by kernel variant (variants.h), the part of every
// bucket inside a tape range, and from those the launch list with each spilling launch's region of
// the ctx's spill memory.  Pure host functions of plain numbers: no HIP call, no handle, so
// tests/native/launch_plan_check.cpp exercises them on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "variants.h"

namespace mh {

// An id list bucketed by kernel variant: ascending ids inside a bucket, the buckets concatenated
// (the order of the tapes' instruction words, and what the device reads as a launch's tape_ids);
// bucket v is ids[off[v], off[v + 1]).
struct Buckets {
    std::vector<uint32_t> ids;
    uint32_t off[kNumVariants + 1] = {};
    struct Range {
        uint32_t first, count;  // ids[first, first + count)
    };
    // the items i of [0, n) that `keep`, as ids base + i in the buckets variant(i)
    template <class Variant, class Keep>
    static Buckets build(uint32_t n, uint32_t base, Variant variant, Keep keep) {
        Buckets b;
        for (uint32_t i = 0; i < n; ++i)
            if (keep(i)) ++b.off[variant(i) + 1];
        for (uint32_t v = 0; v < kNumVariants; ++v) b.off[v + 1] += b.off[v];
        b.ids.resize(b.off[kNumVariants]);
        uint32_t at[kNumVariants];
        std::copy(b.off, b.off + kNumVariants, at);
        for (uint32_t i = 0; i < n; ++i)
            if (keep(i)) b.ids[at[variant(i)]++] = base + i;
        return b;
    }
    // the part of bucket v whose ids lie in [first, first + count)
    Range range(uint32_t v, uint32_t first, uint32_t count) const {
        const uint32_t* e = ids.data() + off[v + 1];
        const uint32_t* lo = std::lower_bound(ids.data() + off[v], e, first);
        const uint32_t* hi = std::lower_bound(lo, e, (uint64_t)first + count);
        return Range{(uint32_t)(lo - ids.data()), (uint32_t)(hi - lo)};
    }
};

// The regions the spilling launches of one call take out of the ctx's spill memory: take() per
// launch while the call is planned, `words` reserved once before anything is queued.  Launches of
// one call may overlap (side streams), so their regions are disjoint.
struct SpillPlan {
    uint64_t words = 0;
    // the launch's region (its offset in words) for `waves` waves of `slots` slots each
    uint64_t take(uint64_t waves, uint32_t slots) {
        const uint64_t at = words;
        words += spill_words(waves, slots);
        return at;
    }
};

struct Launch {
    uint32_t first, count;  // its tape_ids: ids[first, first + count) of the Buckets
    uint32_t variant;
    // the spill variant only (0 otherwise): the most slots a tape of the launch uses, and the
    // launch's region of the SpillPlan
    uint32_t spill_slots;
    uint64_t spill_off;
};
struct LaunchPlan {
    Launch launches[kNumVariants];
    uint32_t n = 0;
    int32_t misfit = -1;  // the first non-empty bucket whose variant cannot address `stride`, or -1
};

// The launches of the ids of `b` inside the tape range [first, first + count) over `rows` rows of a
// buffer of `stride` words per column-limb: one per non-empty bucket.  With `merge` (a short run)
// one per register class instead, the class's first to last non-empty bucket run by the last's
// kernel: the feature sets nest, the register classes do not (a tape's instruction words address
// its class's registers), and a class's buckets are consecutive in the id list.  Only when the
// range holds every id of `b`, though: a bucket cut by the range is no longer contiguous with the
// next, so a sub-range is planned bucket by bucket whatever `merge` says.  `spills` = slots per
// tape id; `waves(rows, n_ids, masks)` = the waves such a launch starts (sieve_launch_waves).
template <class Waves>
LaunchPlan plan_launches(const Buckets& b, uint32_t first, uint32_t count, uint64_t rows,
                         bool merge, bool masks, uint64_t stride, const uint32_t* spills,
                         SpillPlan& spill, Waves waves) {
    LaunchPlan p;
    Buckets::Range r[kNumVariants];
    size_t inside = 0;
    for (uint32_t v = 0; v < kNumVariants; ++v) {
        r[v] = b.range(v, first, count);
        inside += r[v].count;
        if (r[v].count && p.misfit < 0 && !variant_fits(v, stride)) p.misfit = (int32_t)v;
    }
    merge = merge && inside == b.ids.size();
    for (uint32_t v = 0; v < kNumVariants; ++v) {
        if (!r[v].count) continue;
        uint32_t last = v;
        if (merge)
            for (uint32_t u = v + 1; u < (v / kClassVariants + 1) * kClassVariants; ++u)
                if (r[u].count) last = u;
        Launch l{r[v].first, r[last].first + r[last].count - r[v].first, last, 0, 0};
        if (last == kSpillVariant) {
            for (uint32_t i = l.first; i < l.first + l.count; ++i)
                l.spill_slots = std::max(l.spill_slots, spills[b.ids[i]]);
            l.spill_off = spill.take(waves(rows, l.count, masks), l.spill_slots);
        }
        p.launches[p.n++] = l;
        v = last;
    }
    return p;
}

}  // namespace mh
