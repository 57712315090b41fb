// The planner of a batched query round (csrc/batch_plan.h) checked on the host: a stand-alone
// program, built with AddressSanitizer + UBSan by tests/test_batch_plan.py.  For every set of job
// shapes the block tables must cover every (segment, row block, tape slice) exactly once, the
// slices of a segment must partition its tape list the way sieve_body cuts it, segments must be
// grouped by register class with the class's widest feature set, and generator workgroups by
// form.  Prints "cases=N" and exits 0, or prints the failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "batch_plan.h"

using namespace mh::batch;

static int g_cases = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

static void check(const std::vector<JobShape>& jobs) {
    ++g_cases;
    const Plan p = plan(jobs.data(), (uint32_t)jobs.size());
    // --- generator: every (job, row block) of a job with rows exactly once, in its form's launch
    CHECK(p.gen_launches.size() <= kForms);
    std::set<std::pair<uint32_t, uint32_t>> gen_seen;
    uint32_t gen_next = 0, last_form = 0;
    for (size_t li = 0; li < p.gen_launches.size(); ++li) {
        const GenLaunch& l = p.gen_launches[li];
        CHECK(l.count > 0 && l.first == gen_next && l.form < kForms);
        CHECK(li == 0 || l.form > last_form);  // one launch per form
        last_form = l.form;
        gen_next += l.count;
        CHECK(l.lds_bytes <= kGenLdsBytes);
        const uint32_t per = l.form == kFormMem ? kGenRowsPerBlockMem : kGenRowsPerBlock;
        for (uint32_t i = l.first; i < l.first + l.count; ++i) {
            const GenEntry& e = p.gen_blocks[i];
            CHECK(e.job < jobs.size());
            const JobShape& s = jobs[e.job];
            CHECK(gen_form(s.gen_n_cols, s.gen_span_words) == l.form);
            CHECK((uint64_t)e.block * per < s.count);
            const uint64_t need = l.form == kFormStaged ? gen_staged_bytes(s.gen_n_cols, s.gen_span_words)
                                  : l.form == kFormLds  ? gen_lds_bytes(s.gen_n_cols) : 0;
            CHECK(need <= l.lds_bytes);
            CHECK(gen_seen.insert({e.job, e.block}).second);
        }
    }
    CHECK(gen_next == p.gen_blocks.size());
    size_t gen_want = 0;
    for (const JobShape& s : jobs) {
        const uint32_t per =
            gen_form(s.gen_n_cols, s.gen_span_words) == kFormMem ? kGenRowsPerBlockMem : kGenRowsPerBlock;
        gen_want += ceil_div(s.count, per);
    }
    CHECK(gen_seen.size() == gen_want);
    // --- interpreter segments: every nonempty bucket of a job with rows in exactly one segment
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> bucket_seg;  // (job, bucket) -> segment
    for (uint32_t si = 0; si < p.segments.size(); ++si) {
        const Segment& g = p.segments[si];
        CHECK(g.job < jobs.size());
        const JobShape& s = jobs[g.job];
        CHECK(s.count > 0 && g.first_bucket <= g.last_bucket && g.last_bucket < kInterpVariants);
        CHECK(g.first_bucket / 4 == g.last_bucket / 4);  // never across register classes
        CHECK(s.whole || g.first_bucket == g.last_bucket);
        CHECK(s.n_ids[g.first_bucket] > 0 && s.n_ids[g.last_bucket] > 0);
        uint32_t n = 0;
        for (uint32_t v = g.first_bucket; v <= g.last_bucket; ++v) {
            if (!s.n_ids[v]) continue;
            n += s.n_ids[v];
            CHECK(bucket_seg.insert({{g.job, v}, si}).second);
        }
        CHECK(n == g.n_ids);
        CHECK(g.ny >= 1 && g.ny <= g.n_ids);
    }
    for (uint32_t j = 0; j < jobs.size(); ++j)
        for (uint32_t v = 0; v < kInterpVariants; ++v)
            CHECK((bucket_seg.count({j, v}) == 1) == (jobs[j].count > 0 && jobs[j].n_ids[v] > 0));
    // --- launches: one per register class present; every (segment, row block, slice) exactly once
    CHECK(p.launches.size() <= kClasses);
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> seen;
    std::set<uint32_t> classes;
    uint32_t next = 0;
    for (const SieveLaunch& l : p.launches) {
        CHECK(l.count > 0 && l.first == next && l.variant < kInterpVariants);
        CHECK(classes.insert(l.variant / 4).second);
        next += l.count;
        uint32_t widest = 0;
        uint64_t row_blocks = 0;
        std::set<uint32_t> segs;
        for (uint32_t i = l.first; i < l.first + l.count; ++i) {
            const BlockEntry& e = p.blocks[i];
            CHECK(e.seg < p.segments.size());
            const Segment& g = p.segments[e.seg];
            CHECK(g.last_bucket / 4 == l.variant / 4);
            CHECK(g.last_bucket <= l.variant);  // feature sets nest: the launch's covers it
            CHECK(e.ny == g.ny && e.y < e.ny);
            CHECK((uint64_t)e.block * kRowsPerBlock < jobs[g.job].count);
            CHECK(seen.insert(std::make_tuple(e.seg, e.block, e.y)).second);
            widest = g.last_bucket > widest ? g.last_bucket : widest;
            if (segs.insert(e.seg).second) row_blocks += ceil_div(jobs[g.job].count, kRowsPerBlock);
        }
        CHECK(widest == l.variant);
        // launch_block's rule: a launch short of a workgroup per CU splits the tape lists
        for (uint32_t si : segs) {
            const Segment& g = p.segments[si];
            const uint64_t want = row_blocks < kMinBlocks ? (kMinBlocks + row_blocks - 1) / row_blocks : 1;
            CHECK(g.ny == (g.n_ids < want ? g.n_ids : want));
        }
    }
    CHECK(next == p.blocks.size());
    size_t want_blocks = 0;
    for (uint32_t si = 0; si < p.segments.size(); ++si) {
        const Segment& g = p.segments[si];
        CHECK(bucket_seg.count({g.job, g.first_bucket}));
        want_blocks += (size_t)g.ny * ceil_div(jobs[g.job].count, kRowsPerBlock);
        // sieve_body's cut of the tape list: the slices partition [0, n_ids) without a gap
        uint32_t at = 0;
        for (uint32_t y = 0; y < g.ny; ++y) {
            const uint32_t lo = (uint32_t)((uint64_t)g.n_ids * y / g.ny);
            const uint32_t hi = (uint32_t)((uint64_t)g.n_ids * (y + 1) / g.ny);
            CHECK(lo == at && hi > lo);
            at = hi;
        }
        CHECK(at == g.n_ids);
    }
    CHECK(seen.size() == want_blocks);
}

static JobShape job(uint64_t count, uint32_t variant, uint32_t n_ids, bool whole = true,
                    uint32_t n_cols = 4, uint32_t span = 16) {
    JobShape s;
    s.count = count;
    s.n_ids[variant] = n_ids;
    s.whole = whole;
    s.gen_n_cols = n_cols;
    s.gen_span_words = span;
    return s;
}

int main() {
    const uint64_t counts[] = {1, 63, 64, 65, 4096};
    const uint32_t tapes[] = {1, 64, 65, 130};
    check({});  // 0 jobs
    {
        const Plan p = plan(nullptr, 0);
        CHECK(p.launches.empty() && p.gen_launches.empty() && p.blocks.empty());
    }
    // every count x tape-list length, alone and as one batch
    std::vector<JobShape> all;
    for (uint64_t c : counts)
        for (uint32_t t : tapes) {
            check({job(c, 4, t)});
            all.push_back(job(c, (uint32_t)(all.size() % kInterpVariants), t));
        }
    check(all);
    // a single full first round is cut like launch_block cuts it: 64 row blocks x 4 slices
    {
        const std::vector<JobShape> one{job(4096, 8, 130)};
        const Plan p = plan(one.data(), 1);
        CHECK(p.segments.size() == 1 && p.segments[0].ny == 4 && p.blocks.size() == 256);
    }
    // register classes and feature sets: a whole set's class is one segment with the widest
    // bucket; a sub-range keeps one segment per bucket; the launch takes the widest of all
    {
        JobShape a = job(4096, 0, 3);
        a.n_ids[2] = 5;   // class 0: asm-only + keccak
        a.n_ids[9] = 7;   // class 2: complex
        JobShape b = job(65, 1, 2, false);
        b.n_ids[3] = 1;   // class 0, a sub-range: two segments
        b.n_ids[4] = 70;  // class 1
        JobShape c = job(0, 5, 9);  // no rows: nothing at all
        JobShape d = job(64, 11, 1);
        d.n_ids[8] = 1;
        check({a, b, c, d});
        const std::vector<JobShape> js{a, b, c, d};
        const Plan p = plan(js.data(), 4);
        CHECK(p.launches.size() == 3);
        CHECK(p.launches[0].variant == 3 && p.launches[1].variant == 4 && p.launches[2].variant == 11);
        CHECK(p.segments.size() == 6);
        CHECK(p.segments[0].job == 0 && p.segments[0].first_bucket == 0 &&
              p.segments[0].last_bucket == 2 && p.segments[0].n_ids == 8);
    }
    // generator forms: staged LDS, unstaged LDS (the span does not fit), in memory (too many
    // columns, or none), mixed in one batch with different LDS needs
    {
        CHECK(gen_form(4, 16) == kFormStaged);
        CHECK(gen_form(100, 12000) == kFormLds);   // 25600 + 48000 B > 64 KiB, 25600 <= 48 KiB
        CHECK(gen_form(200, 0) == kFormStaged);    // 51200 B of slots alone fit 64 KiB staged
        CHECK(gen_form(200, 4000) == kFormMem);    // 67200 B staged, 51200 B of slots > 48 KiB
        CHECK(gen_form(0, 0) == kFormMem);
        CHECK(gen_form(192, 4096) == kFormStaged); // 49152 + 16384 = 64 KiB exactly
        CHECK(gen_form(192, 4097) == kFormLds);
        CHECK(gen_form(193, 4097) == kFormMem);
        std::vector<JobShape> js;
        js.push_back(job(4096, 0, 1, true, 4, 16));
        js.push_back(job(65, 0, 1, true, 100, 12000));
        js.push_back(job(257, 0, 1, true, 200, 4000));
        js.push_back(job(1, 0, 1, true, 40, 900));
        js.push_back(job(63, 0, 1, true, 0, 0));
        check(js);
        const Plan p = plan(js.data(), (uint32_t)js.size());
        CHECK(p.gen_launches.size() == 3);
        CHECK(p.gen_launches[0].lds_bytes == gen_staged_bytes(40, 900));
        CHECK(p.gen_launches[1].lds_bytes == gen_lds_bytes(100));
        CHECK(p.gen_launches[2].lds_bytes == 0 && p.gen_launches[2].count == 2 + 1);
    }
    // 256 jobs (MH_ROUND_MANY_MAX) of mixed shapes
    {
        std::vector<JobShape> js;
        for (uint32_t i = 0; i < 256; ++i) {
            JobShape s = job(counts[i % 5], i % kInterpVariants, tapes[i % 4], i % 3 != 0,
                             1 + (i * 7) % 220, (i * 131) % 14000);
            if (i % 4 == 1) s.n_ids[(i + 5) % kInterpVariants] = 1 + i % 9;
            js.push_back(s);
        }
        check(js);
    }
    std::printf("cases=%d\n", g_cases);
    return 0;
}
