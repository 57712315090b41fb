// Planner of a batched query round (mh_query_round_many, capi.cpp): turns the jobs' shapes into
// the block tables and the launch lists the batch kernels read (sieve_kernels.hip
// sieve_batch_kernel, generate.hip guided_batch_*).  A pure host function of plain numbers: no
// HIP call, no handle, so tests/native/batch_plan_check.cpp exercises it on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "variants.h"

namespace mh {
namespace batch {

constexpr uint32_t kRowsPerBlock = 64;   // one-wave workgroups: the short-run shape (kShortRows)
constexpr uint32_t kMaxRows = 4096;      // a job's rows at most (sieve_kernels.hip kShortRows)
constexpr uint32_t kGenRowsPerBlock = 64;    // LDS generator forms (generate.hip kLdsRows)
constexpr uint32_t kGenRowsPerBlockMem = 256;  // in-memory form (generate.hip kBlock)
// NR class x feature class, then a fourth class of four (variants.h): the table variants 12..14,
// which never batch (a round's tapes hold no lookup), and the spill variant 15, whose segments
// share one spill region indexed by the launch's workgroup
constexpr uint32_t kInterpVariants = kNumVariants;
constexpr uint32_t kClasses = kNumClasses;
constexpr uint32_t kForms = 3;
constexpr uint32_t kMinBlocks = 256;     // launch_block's target: a workgroup per CU

// The guided generator's kernel forms and the rule that picks one (launch_generate_guided and the
// batched launches share it, so a job's rows are written by the same code either way).
enum GenForm : uint32_t { kFormStaged = 0, kFormLds = 1, kFormMem = 2 };
constexpr uint64_t kGenLdsBytes = 64 * 1024;  // LDS of one generator workgroup at most
inline uint64_t gen_lds_bytes(uint32_t n_cols) { return (uint64_t)n_cols * kGenRowsPerBlock * 4; }
inline uint64_t gen_staged_bytes(uint32_t n_cols, uint32_t span_words) {
    return gen_lds_bytes(n_cols) + (uint64_t)span_words * 4;
}
inline GenForm gen_form(uint32_t n_cols, uint32_t span_words) {
    if (n_cols && gen_staged_bytes(n_cols, span_words) <= kGenLdsBytes) return kFormStaged;
    if (n_cols && gen_lds_bytes(n_cols) <= 48 * 1024) return kFormLds;
    return kFormMem;
}

// What the planner needs of one job.
struct JobShape {
    uint64_t count = 0;                      // rows, <= kMaxRows
    // the job's tapes per interpreter bucket (variants.h variant_of), inside its tape range
    uint32_t n_ids[kInterpVariants] = {};
    // the job runs its whole tape set: a register class's buckets are then one contiguous id range
    // (mh_run_async's merged short run), else every bucket is a range of its own
    bool whole = false;
    uint32_t gen_n_cols = 0, gen_span_words = 0;  // the guide, for gen_form / the LDS size
};

// One contiguous id range of one job: the unit that gets a KParams on the device.
struct Segment {
    uint32_t job;
    uint32_t first_bucket;   // the range starts at this bucket's first id inside the job's range
    uint32_t last_bucket;    // and ends with this bucket's last (== first_bucket unless merged)
    uint32_t n_ids;
    uint32_t ny;             // tape slices (the part of gridDim.y)
};
// One workgroup of an interpreter launch ({x, y} = segment's row block, tape slice y of ny).
struct BlockEntry {
    uint32_t seg, block, y, ny;
};
// One workgroup of a generator launch.
struct GenEntry {
    uint32_t job, block;
};
struct SieveLaunch {
    uint32_t variant;        // the register class's widest feature set among its segments
    uint32_t first, count;   // its slice of Plan::blocks
};
struct GenLaunch {
    uint32_t form;
    uint32_t first, count;   // its slice of Plan::gen_blocks
    uint64_t lds_bytes;      // dynamic LDS: the largest any of its jobs needs
};
struct Plan {
    std::vector<Segment> segments;
    std::vector<BlockEntry> blocks;
    std::vector<GenEntry> gen_blocks;
    std::vector<SieveLaunch> launches;    // at most kClasses
    std::vector<GenLaunch> gen_launches;  // at most kForms
};

inline Plan plan(const JobShape* jobs, uint32_t n_jobs) {
    Plan p;
    // generator: one launch per form present, a {job, row block} entry per workgroup
    for (uint32_t f = 0; f < kForms; ++f) {
        GenLaunch g{f, (uint32_t)p.gen_blocks.size(), 0, 0};
        const uint32_t per = f == kFormMem ? kGenRowsPerBlockMem : kGenRowsPerBlock;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            const JobShape& s = jobs[j];
            if (s.count == 0 || gen_form(s.gen_n_cols, s.gen_span_words) != f) continue;
            const uint32_t nb = (uint32_t)((s.count + per - 1) / per);
            for (uint32_t b = 0; b < nb; ++b) p.gen_blocks.push_back(GenEntry{j, b});
            const uint64_t lds = f == kFormStaged ? gen_staged_bytes(s.gen_n_cols, s.gen_span_words)
                                 : f == kFormLds  ? gen_lds_bytes(s.gen_n_cols) : 0;
            g.lds_bytes = std::max(g.lds_bytes, lds);
        }
        g.count = (uint32_t)p.gen_blocks.size() - g.first;
        if (g.count) p.gen_launches.push_back(g);
    }
    // interpreter: one launch per register class; feature sets nest, register classes do not
    for (uint32_t c = 0; c < kClasses; ++c) {
        const uint32_t seg_first = (uint32_t)p.segments.size();
        uint32_t widest = 0;
        uint64_t row_blocks = 0;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            const JobShape& s = jobs[j];
            if (s.count == 0) continue;
            const uint64_t nb = (s.count + kRowsPerBlock - 1) / kRowsPerBlock;
            for (uint32_t v = kClassVariants * c; v < kClassVariants * (c + 1); ++v) {
                if (!s.n_ids[v]) continue;
                Segment g{j, v, v, s.n_ids[v], 1};
                if (s.whole)
                    for (uint32_t u = v + 1; u < kClassVariants * (c + 1); ++u)
                        if (s.n_ids[u]) {
                            g.last_bucket = u;
                            g.n_ids += s.n_ids[u];
                        }
                widest = std::max(widest, g.last_bucket);
                p.segments.push_back(g);
                row_blocks += nb;
                if (s.whole) break;
            }
        }
        if (p.segments.size() == seg_first) continue;
        // launch_block's rule over the whole launch: fewer row blocks than CUs split every
        // segment's tape list until the chip has ~kMinBlocks workgroups
        const uint64_t want = row_blocks < kMinBlocks ? (kMinBlocks + row_blocks - 1) / row_blocks : 1;
        SieveLaunch l{widest, (uint32_t)p.blocks.size(), 0};
        for (uint32_t si = seg_first; si < p.segments.size(); ++si) {
            Segment& g = p.segments[si];
            g.ny = (uint32_t)std::min<uint64_t>(g.n_ids, want);
            const uint32_t nb =
                (uint32_t)((jobs[g.job].count + kRowsPerBlock - 1) / kRowsPerBlock);
            for (uint32_t y = 0; y < g.ny; ++y)
                for (uint32_t b = 0; b < nb; ++b) p.blocks.push_back(BlockEntry{si, b, y, g.ny});
        }
        l.count = (uint32_t)p.blocks.size() - l.first;
        p.launches.push_back(l);
    }
    return p;
}

}  // namespace batch
}  // namespace mh
