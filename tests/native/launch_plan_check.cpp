// The bucketed id list and the planner of the interpreter's direct launches (csrc/launch_plan.h)
// checked on the host: a stand-alone program, built with AddressSanitizer + UBSan by
// tests/test_launch_plan.py.  Buckets are built from a fixed variant function over small id sets;
// for every tape range (empty, one id, from and to every bucket's first and last id, the whole
// set) x merge on / off x masks on / off x 1 / 64 / 65 / 4096 / 4097 rows x a stride below and at
// 2^30: every id of the range is in exactly one launch and no other id in any; a launch is one
// contiguous run of the id list, ascending inside a bucket; unmerged, a launch's variant is its
// bucket; merged over a range that holds the whole list, a launch spans its register class's first
// to last non-empty bucket with the last's variant and never crosses a class (a merged launch over
// a bucket cut by the range would take in ids outside it: such a range is planned unmerged); the
// spill variant's launches, and no others, take regions of spill_words(waves, most slots of their
// ids), back to back in the SpillPlan; the capacity verdict is the first non-empty bucket that
// fails variant_fits.  Prints "cases=N" and exits 0, or prints the failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_plan.h"

using namespace mh;

static int g_cases = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

// a stand-in for sieve_launch_waves: any fixed function of the launch's shape
static uint64_t waves(uint64_t rows, uint32_t n_ids, bool masks) {
    if (rows == 0 || n_ids == 0) return 0;
    const uint64_t blocks = (rows + 63) / 64;
    return blocks * (masks ? n_ids : blocks < 8 ? std::min<uint64_t>(n_ids, 8 / blocks) : 1);
}

// A tape set: the variant of every item, which items are kept, the ids' base; a spilling tape's
// slots are a fixed function of its id.
struct Set {
    std::vector<uint32_t> variant;
    std::vector<char> keep;
    uint32_t base = 0;
    Buckets b;
    std::vector<uint32_t> spills;  // [base + items]
};

static Set make(const std::vector<uint32_t>& variant, uint32_t base = 0, uint32_t drop_every = 0) {
    Set s;
    s.variant = variant;
    s.base = base;
    const uint32_t n = (uint32_t)variant.size();
    for (uint32_t i = 0; i < n; ++i) s.keep.push_back(!(drop_every && i % drop_every == 1));
    s.spills.assign(base + n, 0);
    for (uint32_t i = 0; i < n; ++i)
        if (variant[i] == kSpillVariant) s.spills[base + i] = 1 + (i * 5) % 7;
    s.b = Buckets::build(n, base, [&](uint32_t i) { return s.variant[i]; },
                         [&](uint32_t i) { return s.keep[i] != 0; });
    // every kept item once, in its variant's bucket, ascending; nothing else
    CHECK(s.b.off[0] == 0 && s.b.off[kNumVariants] == s.b.ids.size());
    size_t kept = 0;
    for (uint32_t i = 0; i < n; ++i) kept += s.keep[i] != 0;
    CHECK(s.b.ids.size() == kept);
    for (uint32_t v = 0; v < kNumVariants; ++v) {
        CHECK(s.b.off[v] <= s.b.off[v + 1]);
        for (uint32_t q = s.b.off[v]; q < s.b.off[v + 1]; ++q) {
            const uint32_t id = s.b.ids[q];
            CHECK(id >= base && id - base < n && s.keep[id - base] && s.variant[id - base] == v);
            CHECK(q == s.b.off[v] || s.b.ids[q - 1] < id);
        }
    }
    return s;
}

static uint32_t bucket_at(const Buckets& b, uint32_t q) {
    uint32_t v = 0;
    while (q >= b.off[v + 1]) ++v;
    return v;
}

static void check(const Set& s, uint32_t first, uint32_t count, uint64_t rows, bool merge,
                  bool masks, uint64_t stride) {
    ++g_cases;
    const Buckets& b = s.b;
    const uint32_t n = (uint32_t)b.ids.size();
    // range(): the ids of bucket v inside [first, first + count), by brute force
    uint32_t in_bucket[kNumVariants] = {}, inside = 0;
    int32_t want_misfit = -1;
    for (uint32_t v = 0; v < kNumVariants; ++v) {
        const Buckets::Range r = b.range(v, first, count);
        CHECK(r.first >= b.off[v] && r.first + r.count <= b.off[v + 1]);
        for (uint32_t q = b.off[v]; q < b.off[v + 1]; ++q) {
            const bool in = b.ids[q] >= first && (uint64_t)b.ids[q] < (uint64_t)first + count;
            CHECK(in == (q >= r.first && q < r.first + r.count));
        }
        in_bucket[v] = r.count;
        inside += r.count;
        if (r.count && want_misfit < 0 && !variant_fits(v, stride)) want_misfit = (int32_t)v;
    }
    SpillPlan spill;
    const uint64_t before = spill.take(3, 2);  // an earlier launch of the call holds a region
    CHECK(before == 0);
    uint64_t next_region = spill.words;
    const LaunchPlan p = plan_launches(b, first, count, rows, merge, masks, stride,
                                       s.spills.data(), spill, waves);
    CHECK(p.misfit == want_misfit);
    CHECK(p.n <= kNumVariants);
    const bool merged = merge && inside == n;
    std::vector<uint32_t> times(n, 0);
    uint32_t at = 0, n_want = 0;
    for (uint32_t k = 0; k < p.n; ++k) {
        const Launch& l = p.launches[k];
        CHECK(l.count > 0 && l.first >= at && (uint64_t)l.first + l.count <= n);
        at = l.first + l.count;
        const uint32_t v0 = bucket_at(b, l.first), v1 = bucket_at(b, at - 1);
        uint32_t slots = 0;
        for (uint32_t q = l.first; q < at; ++q) {
            ++times[q];
            CHECK(q == l.first || bucket_at(b, q) != bucket_at(b, q - 1) || b.ids[q - 1] < b.ids[q]);
            slots = std::max(slots, s.spills[b.ids[q]]);
        }
        CHECK(l.variant == v1 && v0 / kClassVariants == v1 / kClassVariants);
        if (!merged) {
            CHECK(v0 == v1);
        } else {  // the class's first to last non-empty bucket, whole
            CHECK(l.first == b.off[v0] && at == b.off[v1 + 1]);
            for (uint32_t u = v0 / kClassVariants * kClassVariants; u < v0; ++u) CHECK(!in_bucket[u]);
            for (uint32_t u = v1 + 1; u < (v1 / kClassVariants + 1) * kClassVariants; ++u)
                CHECK(!in_bucket[u]);
        }
        if (l.variant == kSpillVariant) {  // regions back to back: disjoint, and they sum to words
            CHECK(l.spill_slots == slots && l.spill_off == next_region);
            next_region += spill_words(waves(rows, l.count, masks), slots);
        } else {
            CHECK(l.spill_slots == 0 && l.spill_off == 0);
        }
    }
    CHECK(spill.words == next_region);
    for (uint32_t q = 0; q < n; ++q) {
        const bool in = b.ids[q] >= first && (uint64_t)b.ids[q] < (uint64_t)first + count;
        CHECK(times[q] == (in ? 1u : 0u));
    }
    for (uint32_t c = 0; c < kNumClasses; ++c) {
        uint32_t nonempty = 0;
        for (uint32_t v = c * kClassVariants; v < (c + 1) * kClassVariants; ++v)
            nonempty += in_bucket[v] ? 1 : 0;
        n_want += merged ? (nonempty ? 1 : 0) : nonempty;
    }
    CHECK(p.n == n_want);
}

static void check_set(const Set& s) {
    const Buckets& b = s.b;
    const uint32_t n_items = (uint32_t)s.variant.size(), end = s.base + n_items;
    std::vector<std::pair<uint32_t, uint32_t>> ranges = {
        {s.base, 0}, {end, 0}, {0, 0}, {s.base, n_items}, {0, end}, {0, end + 3}};
    for (uint32_t i = 0; i < n_items; i += 3) ranges.push_back({s.base + i, 1});  // one id
    for (uint32_t v = 0; v < kNumVariants; ++v) {
        if (b.off[v] == b.off[v + 1]) continue;
        const uint32_t lo = b.ids[b.off[v]], hi = b.ids[b.off[v + 1] - 1];
        ranges.push_back({lo, hi - lo + 1});      // from the bucket's first to its last id
        ranges.push_back({lo, end - lo});         // from its first id on
        ranges.push_back({s.base, hi + 1 - s.base});  // up to its last id
        ranges.push_back({lo + 1, hi - lo});      // and the same cut one id short at either end
        ranges.push_back({s.base, hi - s.base});
    }
    for (const auto& r : ranges)
        for (uint64_t rows : {1ull, 64ull, 65ull, 4096ull, 4097ull})
            for (int merge = 0; merge < 2; ++merge)
                for (int masks = 0; masks < 2; ++masks)
                    for (uint64_t stride : {kLoadvarMaxCapacity - 1, kLoadvarMaxCapacity})
                        check(s, r.first, r.second, rows, merge != 0, masks != 0, stride);
}

int main() {
    std::vector<uint32_t> mixed, spill_only(5, kSpillVariant);
    for (uint32_t i = 0; i < 45; ++i) mixed.push_back((i * 7 + 3) % kNumVariants);
    check_set(make({}));                      // all variants empty
    check_set(make({9}));                     // one tape
    check_set(make(mixed));                   // every bucket
    check_set(make(mixed, 0, 3));             // some items dropped (the JIT's, the split tapes)
    check_set(make(mixed, 45));               // parts: ids after the tapes'
    check_set(make(spill_only));              // only the spill bucket
    check_set(make(spill_only, 7, 2));
    // a class with only its first and fourth bucket: class 1, and the table / spill class
    check_set(make({4, 7, 7, 4, 4, 7}));
    check_set(make({12, 15, 15, 12, 0, 15, 12}));
    // only the asm-only variants (0, 4, 8) take a stride of 2^30
    {
        const Set s = make({0, 4, 8, 4, 0});
        SpillPlan spill;
        CHECK(plan_launches(s.b, 0, 5, 64, true, false, 1ull << 31, s.spills.data(), spill, waves)
                  .misfit == -1);
        const Set t = make({0, 4, 9, 5, 0});
        CHECK(plan_launches(t.b, 0, 5, 64, false, false, kLoadvarMaxCapacity, t.spills.data(),
                            spill, waves).misfit == 5);
        CHECK(plan_launches(t.b, 0, 5, 64, false, false, kLoadvarMaxCapacity - 1, t.spills.data(),
                            spill, waves).misfit == -1);
        CHECK(spill.words == 0);
    }
    std::printf("cases=%d\n", g_cases);
    return 0;
}
