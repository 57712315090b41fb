// Planner of a batched values submission (mh_eval_values_jobs, capi.cpp): turns the jobs' id lists
// and each id's kernel variant into the sorted id list, the segments, the block table and the
// launch list the batch kernels read (sieve_kernels.hip sieve_batch_kernel in values mode).  A pure
// host function of plain numbers: no HIP call, no handle, so tests/native/values_plan_check.cpp
// exercises it on the CPU.
//
// A job is one row under one tape set: its listed tapes, in any order and with repeats, become
// slots.  The slots of a job are sorted by (variant, tape id, position) -- sieve_body's chunk
// formation needs a launch's ids ascending -- and every (job, variant) run of them is a segment:
// the unit that gets a KParams on the device.  Slot s holds the value of the job's list position
// pos[s]; the kernel writes it at value word 8 s of the submission's value block.  One launch per
// variant present, table variants (12..14) included, so a tape runs the kernel the single calls
// (mh_eval_values / mh_eval_values_many / mh_eval_values_tables) run it with: those sort their one
// list with this planner too (capi.cpp eval_values_rows: a single job, a direct launch per segment
// planned by launch_plan.h).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "batch_plan.h"
#include "variants.h"

namespace mh {
namespace values {

// (variants.h) without spill code: 0..11 table-free, 12..14 table; the spill variant after them
constexpr uint32_t kVariants = kSpillVariant;
constexpr uint32_t kAllVariants = kNumVariants;
constexpr uint32_t kJobsMax = 256;    // MH_VALUES_JOBS_MAX
constexpr uint32_t kMinBlocks = 256;  // launch_block's target: a workgroup per CU

// What the planner needs of one job: its id list and the variant of every listed id.
struct JobShape {
    const uint32_t* ids = nullptr;
    const uint32_t* variants = nullptr;  // [n], each < kAllVariants
    uint32_t n = 0;
};

// One (job, variant) run of slots.
struct Segment {
    uint32_t job;
    uint32_t variant;
    uint32_t first;   // its first slot
    uint32_t n_ids;
    uint32_t ny;      // tape slices: workgroups of the segment (1..n_ids)
};
struct Launch {
    uint32_t variant;
    uint32_t first, count;  // its slice of Plan::blocks
};
struct Plan {
    std::vector<uint32_t> ids;        // [slots] the tape id of every slot
    std::vector<uint32_t> pos;        // [slots] the slot's position in its job's list
    std::vector<uint32_t> job_first;  // [n_jobs + 1] job j's slots are [job_first[j], job_first[j + 1])
    std::vector<Segment> segments;    // job-major, variants ascending inside a job
    std::vector<batch::BlockEntry> blocks;  // {segment, row block 0, tape slice, slices}
    std::vector<Launch> launches;     // variants ascending, at most kAllVariants
};

inline Plan plan(const JobShape* jobs, uint32_t n_jobs) {
    Plan p;
    p.job_first.assign((size_t)n_jobs + 1, 0u);
    size_t total = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) total += jobs[j].n;
    p.ids.reserve(total);
    p.pos.reserve(total);
    uint32_t segs_of[kAllVariants] = {};
    std::vector<uint32_t> order;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const JobShape& s = jobs[j];
        p.job_first[j] = (uint32_t)p.ids.size();
        order.resize(s.n);
        for (uint32_t i = 0; i < s.n; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            if (s.variants[a] != s.variants[b]) return s.variants[a] < s.variants[b];
            if (s.ids[a] != s.ids[b]) return s.ids[a] < s.ids[b];
            return a < b;
        });
        for (uint32_t i = 0; i < s.n;) {
            uint32_t k = i;
            while (k < s.n && s.variants[order[k]] == s.variants[order[i]]) ++k;
            const uint32_t v = s.variants[order[i]];
            p.segments.push_back(Segment{j, v, (uint32_t)p.ids.size(), k - i, 1});
            ++segs_of[v];
            for (; i < k; ++i) {
                p.ids.push_back(s.ids[order[i]]);
                p.pos.push_back(order[i]);
            }
        }
    }
    p.job_first[n_jobs] = (uint32_t)p.ids.size();
    // a segment is one row, so one row block: launch_block's rule over the whole launch splits
    // every segment's tape list until the chip has ~kMinBlocks workgroups
    for (uint32_t v = 0; v < kAllVariants; ++v) {
        if (!segs_of[v]) continue;
        const uint32_t want = segs_of[v] < kMinBlocks ? (kMinBlocks + segs_of[v] - 1) / segs_of[v] : 1;
        Launch l{v, (uint32_t)p.blocks.size(), 0};
        for (uint32_t si = 0; si < p.segments.size(); ++si) {
            Segment& g = p.segments[si];
            if (g.variant != v) continue;
            g.ny = std::min(g.n_ids, want);
            for (uint32_t y = 0; y < g.ny; ++y) p.blocks.push_back(batch::BlockEntry{si, 0, y, g.ny});
        }
        l.count = (uint32_t)p.blocks.size() - l.first;
        p.launches.push_back(l);
    }
    return p;
}

}  // namespace values
}  // namespace mh
