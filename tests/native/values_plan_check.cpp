// The planner of a batched values submission (csrc/values_plan.h) checked on the host: a
// stand-alone program, built with AddressSanitizer + UBSan by tests/test_values_plan.py.  For every
// set of jobs: every listed position of a job appears in exactly one slot, inside a segment of the
// job and of the id's variant and in the launch of that variant; a segment's ids ascend (what
// sieve_body's chunk formation needs); the block table covers every (segment, slice) exactly once
// and the slices partition the segment's id list the way sieve_body cuts it; one launch per
// variant present.  Prints "cases=N" and exits 0, or prints the failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "values_plan.h"

using namespace mh::values;
using mh::batch::BlockEntry;

static int g_cases = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

struct Job {
    std::vector<uint32_t> ids, variants;
};

// the variant of a tape id: any fixed function of the id, as a tape set's is
static uint32_t variant_of_id(uint32_t id, uint32_t salt) { return (id * 7 + salt) % kVariants; }

static Job job(const std::vector<uint32_t>& ids, uint32_t salt = 0) {
    Job j;
    j.ids = ids;
    for (uint32_t id : ids) j.variants.push_back(variant_of_id(id, salt));
    return j;
}

static Plan check(const std::vector<Job>& jobs) {
    ++g_cases;
    std::vector<JobShape> shapes(jobs.size());
    size_t total = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        shapes[j].ids = jobs[j].ids.data();
        shapes[j].variants = jobs[j].variants.data();
        shapes[j].n = (uint32_t)jobs[j].ids.size();
        total += jobs[j].ids.size();
    }
    const Plan p = plan(shapes.data(), (uint32_t)shapes.size());
    // --- slots: a permutation of every job's positions, the id kept
    CHECK(p.ids.size() == total && p.pos.size() == total);
    CHECK(p.job_first.size() == jobs.size() + 1 && p.job_first[0] == 0);
    for (size_t j = 0; j < jobs.size(); ++j) {
        CHECK(p.job_first[j + 1] - p.job_first[j] == jobs[j].ids.size());
        std::set<uint32_t> seen;
        for (uint32_t q = p.job_first[j]; q < p.job_first[j + 1]; ++q) {
            CHECK(p.pos[q] < jobs[j].ids.size());
            CHECK(seen.insert(p.pos[q]).second);  // every position exactly once
            CHECK(p.ids[q] == jobs[j].ids[p.pos[q]]);
        }
    }
    // --- segments: tile the slots in order, one (job, variant) each, ids ascending
    uint32_t at = 0;
    std::set<std::pair<uint32_t, uint32_t>> job_variant;
    uint32_t present[kVariants] = {};
    for (const Segment& g : p.segments) {
        CHECK(g.job < jobs.size() && g.variant < kVariants && g.n_ids > 0);
        CHECK(g.first == at);
        CHECK(g.first >= p.job_first[g.job] && g.first + g.n_ids <= p.job_first[g.job + 1]);
        CHECK(job_variant.insert({g.job, g.variant}).second);
        for (uint32_t q = g.first; q < g.first + g.n_ids; ++q) {
            CHECK(jobs[g.job].variants[p.pos[q]] == g.variant);
            CHECK(q == g.first || p.ids[q - 1] <= p.ids[q]);
        }
        CHECK(g.ny >= 1 && g.ny <= g.n_ids);
        // sieve_body's cut of the id list: the slices partition [0, n_ids) without a gap
        uint32_t cut = 0;
        for (uint32_t y = 0; y < g.ny; ++y) {
            const uint32_t lo = (uint32_t)((uint64_t)g.n_ids * y / g.ny);
            const uint32_t hi = (uint32_t)((uint64_t)g.n_ids * (y + 1) / g.ny);
            CHECK(lo == cut && hi > lo);
            cut = hi;
        }
        CHECK(cut == g.n_ids);
        at += g.n_ids;
        ++present[g.variant];
    }
    CHECK(at == total);
    // --- launches: one per variant present, ascending; every (segment, slice) exactly once, in
    // the launch of the segment's variant
    std::set<std::pair<uint32_t, uint32_t>> blocks_seen;
    uint32_t next = 0, n_present = 0;
    for (uint32_t v = 0; v < kVariants; ++v) n_present += present[v] ? 1 : 0;
    CHECK(p.launches.size() == n_present);
    for (size_t li = 0; li < p.launches.size(); ++li) {
        const Launch& l = p.launches[li];
        CHECK(l.variant < kVariants && present[l.variant] && l.count > 0 && l.first == next);
        CHECK(li == 0 || l.variant > p.launches[li - 1].variant);
        next += l.count;
        const uint32_t want =
            present[l.variant] < kMinBlocks ? (kMinBlocks + present[l.variant] - 1) / present[l.variant] : 1;
        for (uint32_t i = l.first; i < l.first + l.count; ++i) {
            const BlockEntry& e = p.blocks[i];
            CHECK(e.seg < p.segments.size());
            const Segment& g = p.segments[e.seg];
            CHECK(g.variant == l.variant);
            CHECK(e.block == 0 && e.ny == g.ny && e.y < e.ny);  // one row: one row block
            CHECK(g.ny == (g.n_ids < want ? g.n_ids : want));
            CHECK(blocks_seen.insert({e.seg, e.y}).second);
        }
    }
    CHECK(next == p.blocks.size());
    size_t want_blocks = 0;
    for (const Segment& g : p.segments) want_blocks += g.ny;
    CHECK(blocks_seen.size() == want_blocks);
    return p;
}

int main() {
    // 0 jobs, and jobs without ids
    {
        const Plan p = plan(nullptr, 0);
        CHECK(p.launches.empty() && p.blocks.empty() && p.segments.empty() && p.ids.empty());
        CHECK(p.job_first.size() == 1 && p.job_first[0] == 0);
        check({});
        const Plan q = check({job({}), job({})});
        CHECK(q.launches.empty() && q.job_first.size() == 3);
    }
    // 1 job: one id; repeats; descending; 64 / 65 / 130 ids of one variant and of all
    {
        const Plan p = check({job({5})});
        CHECK(p.segments.size() == 1 && p.blocks.size() == 1 && p.launches.size() == 1);
        check({job({3, 3, 3})});
        check({job({9, 7, 7, 2, 9, 0})});
        for (uint32_t n : {64u, 65u, 130u}) {
            std::vector<uint32_t> same, all;
            for (uint32_t i = 0; i < n; ++i) {
                same.push_back((n - i) * kVariants);  // descending, one variant
                all.push_back(n - i);
            }
            const Plan one = check({job(same)});
            CHECK(one.segments.size() == 1 && one.segments[0].ny == n);  // a slice per tape
            check({job(all)});
        }
    }
    // repeats keep their own slots, in position order
    {
        const Plan p = check({job({4, 1, 4, 1})});  // variants 13, 7, 13, 7
        CHECK(p.ids == (std::vector<uint32_t>{1, 1, 4, 4}));
        CHECK(p.pos == (std::vector<uint32_t>{1, 3, 0, 2}));
    }
    // a few jobs that share variants: one launch per variant, not per job
    {
        const Plan p = check({job({0, 15, 30}), job({15, 0}), job({1}, 3), job({30, 30, 45})});
        CHECK(p.launches.size() == 2);  // variant_of_id(0 / 15 / 30 / 45, 0) = 0; (1, 3) = 10
        CHECK(p.launches[0].variant == 0 && p.launches[1].variant == 10);
        CHECK(p.segments.size() == 4);
    }
    // 256 jobs (MH_VALUES_JOBS_MAX): one with 65 ids of one variant is not sliced (a workgroup
    // walks all 65, across the 64-tape chunk), mixed lengths and variants
    {
        std::vector<Job> js;
        for (uint32_t i = 0; i < kJobsMax; ++i) {
            std::vector<uint32_t> ids;
            const uint32_t n = i == 7 ? 65 : i % 5;
            for (uint32_t k = 0; k < n; ++k) ids.push_back(i == 7 ? (70 - k) * kVariants : (i * 31 + k * 17) % 97);
            js.push_back(job(ids, i == 7 ? 0 : i % 4));
        }
        check(js);
        std::vector<Job> same;
        for (uint32_t i = 0; i < kJobsMax; ++i) {
            std::vector<uint32_t> ids;
            for (uint32_t k = 0; k < (i == 7 ? 65u : 1u); ++k) ids.push_back((70 - k) * kVariants);
            same.push_back(job(ids));
        }
        const Plan p = check(same);
        CHECK(p.launches.size() == 1 && p.segments[7].n_ids == 65 && p.segments[7].ny == 1);
        CHECK(p.blocks.size() == kJobsMax);
    }
    std::printf("cases=%d\n", g_cases);
    return 0;
}
