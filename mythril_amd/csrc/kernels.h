// Launch interface between the C-ABI layer (capi.cpp) and the kernels (sieve_kernels.hip).  The
// kernel variants' numbering is variants.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mythril_hip.h"
#include "batch_plan.h"
#include "dev_isa.h"
#include "variants.h"

namespace mh {

struct KParams {
    const uint2* insns;          // instruction words (2 x u32 per instruction)
    const mh_dev_tape* tapes;    // per-tape headers
    const uint32_t* consts;      // device constant pool, 8 limbs per entry
    const uint32_t* assign;      // SoA assignment buffer
    const uint32_t* tape_ids;    // the tapes this launch evaluates (one kernel-variant bucket)
    uint64_t capacity;           // column stride in words (>= rows allocated per column)
    uint32_t n_pre;              // columns preloaded into R0..R(n_pre-1)
    uint32_t n_ids;              // entries of tape_ids
    uint32_t result_base;        // results are indexed by tape id - result_base
    uint32_t pad;
    uint64_t row_first, row_count, index_base;
    uint32_t mode;
    unsigned long long* first_hit;  // [tapes of the run]
    unsigned long long* hit_count;  // [tapes of the run]
    uint32_t* values_out;           // parity path: [n_ids][8][row_count] root values, or null
    // conjunct-parallel short runs (capi.cpp mh_run_async): each wave of a part-tape writes its
    // 64-row Bool mask to masks[(tape id - mask_base) * mask_stride + wave of the run] instead
    // of first hits / counts, which the combine kernel then ANDs per split tape
    unsigned long long* masks;
    uint32_t mask_base;
    uint32_t pad2;
    uint64_t mask_stride;           // waves of the run's grid (sieve_mask_stride)
    const uint32_t* tables;         // the table set D_LOOKUP reads (dev_isa.h layout), or null
    // the spill variant only (F_SPILL tapes; null / 0 otherwise): this launch's region of the
    // ctx's spill memory, and the slots every wave owns in it (the maximum over the launch's
    // tapes).  Wave W of the launch -- linear workgroup index of the LAUNCH (not of a batch
    // segment) x waves per workgroup + wave in the workgroup -- keeps slot s, limb k of lane l at
    // word ((W * spill_slots + s) * 8 + k) * 64 + l: 256 contiguous bytes per limb, like a column
    // load.  Lanes of rows outside the run spill there too (nothing is indexed by row).
    uint32_t* spill;
    uint32_t spill_slots;
    uint32_t pad3;
};
hipError_t launch_sieve(const KParams& p, uint32_t variant, hipStream_t stream);
// waves launch_sieve starts for a run of row_count rows over n_ids tapes (what the spill variant's
// region is sized by: launch_plan.h plan_launches takes spill_words(waves, spill_slots) per launch)
uint64_t sieve_launch_waves(uint64_t row_count, uint32_t n_ids, bool masks);
hipError_t launch_generate(uint32_t* assign, uint64_t stride, uint64_t rows, uint32_t n_vars,
                           uint64_t seed, uint64_t base, hipStream_t stream);
// Device form of mh_guide (pointers into one device buffer owned by the mh_assign).
struct KGuide {
    uint32_t n_cols, n_sets;
    uint32_t n_value_sets;      // sets [0, n_value_sets) hold no copy entry
    const uint32_t* width;      // [n_cols]
    const uint32_t* pool_off;   // [n_cols + 1]
    const uint32_t* pool;       // x 8 limbs
    const uint32_t* set_prob;   // [n_sets]
    const uint32_t* set_off;    // [n_sets + 1]
    const uint32_t* alt_off;    // [n_alts + 1]
    const uint32_t* entry_col;  // [n_entries]
    const uint32_t* entry_val;  // x 8 limbs
    // set_prob | set_off | alt_off | entry_col lie back to back from set_prob (span_words
    // words): the generator stages them in LDS when they fit
    uint32_t span_words;
};
hipError_t launch_generate_guided(uint32_t* assign, uint64_t stride, uint64_t first,
                                  uint64_t count, uint64_t seed, uint64_t base, const KGuide& g,
                                  hipStream_t stream);
// One domain column of an enumeration (mh_assign_enumerate; enumerate.hip), 64 bytes, on the
// device once per domain set; a list's values are 8-limb entries of the set's value block.
struct KDomain {
    uint64_t size;      // values in the domain (> 0 in any launch)
    uint32_t col;       // the buffer column written
    uint32_t kind;      // MH_DOMAIN_*
    uint32_t lo[8];     // an interval's first value
    uint32_t list_off;  // a list's first entry in the value block
    uint32_t pad[3];
};
static_assert(sizeof(KDomain) == 64, "KDomain is packed by words (capi.cpp)");
// rows [first, first + count) of the buffer: the cross product's rows base.. in order; the caller
// has checked every column and the row range against the buffer
hipError_t launch_enumerate(uint32_t* assign, uint64_t stride, uint64_t first, uint64_t count,
                            uint64_t base, const KDomain* doms, uint32_t n_doms,
                            const uint32_t* list_vals, hipStream_t stream);
// A batched round (mh_query_round_many; the tables are batch_plan.h's, on the device, read only).
// Interpreter: workgroup i of the launch runs blocks[i] = {segment, row block, tape slice, slices}
// with segs[segment]; `variant` serves every segment of the launch.  A round's launches are
// table-free (`variant` < kFirstTableVariant, or kSpillVariant with segments that carry their
// part of the launch's spill region); mh_eval_values_jobs (values_plan.h: one-row
// segments in values mode, row block 0) also launches the table variants, whose segments each
// carry their own `tables`.
hipError_t launch_sieve_batch(const KParams* segs, const batch::BlockEntry* blocks,
                              uint32_t n_blocks, uint32_t variant, hipStream_t stream);
// Generator: what launch_generate_guided takes, per job (rows [0, count) of the buffer).
struct GenJob {
    uint32_t* assign;
    uint64_t stride, count, seed, base;
    KGuide g;
};
// workgroup i writes row block blocks[i].block of jobs[blocks[i].job] with the kernel of `form`
// (batch::GenForm: every job of the launch has that form, batch::gen_form)
hipError_t launch_generate_guided_batch(const GenJob* jobs, const batch::GenEntry* blocks,
                                        uint32_t n_blocks, uint32_t form, uint64_t lds_bytes,
                                        hipStream_t stream);
// One job's slice of the batch's device result block, first_hit[tc] | hit_count[tc] |
// rows[tc][n_cols][8], and the buffer its witness rows are read from.
struct ResultJob {
    uint64_t* first_hit;     // hit_count = first_hit + tc, rows = first_hit + 2 tc
    const uint32_t* assign;
    uint64_t stride, index_base;
    uint32_t tc, n_cols;
};
// every job's first_hit = MH_NO_HIT and hit_count = 0: one launch, a workgroup per job
hipError_t launch_results_reset_batch(const ResultJob* jobs, uint32_t n_jobs, hipStream_t stream);
// every job's witness rows (launch_witness_rows per job): one launch, grid (tapes, jobs)
hipError_t launch_witness_rows_batch(const ResultJob* jobs, uint32_t n_jobs, uint32_t max_tc,
                                     hipStream_t stream);
// first_hit[0..n) = MH_NO_HIT, hit_count[0..n) = 0 in one launch (either may be null)
hipError_t launch_results_reset(uint64_t* first_hit, uint64_t* hit_count, uint32_t n,
                                hipStream_t stream);
// each tape's witness row (mh_run_rows): out[t][w] = column word w (column w / 8, limb w % 8) of
// the buffer row first_hit[t] - index_base, zero for a tape without a hit
hipError_t launch_witness_rows(const uint32_t* assign, uint64_t stride, const uint64_t* first_hit,
                               uint32_t n_tapes, uint64_t index_base, uint32_t n_cols,
                               uint32_t* out, hipStream_t stream);
// waves a run of row_count rows launches (the masks' row stride of a conjunct-parallel run)
uint64_t sieve_mask_stride(uint64_t row_count);
// per split tape i (split[3i] = tape id, split[3i+1] = its first part's id, whose masks are
// row id - mask_base, split[3i+2] = parts): the AND of its parts' masks per wave -> atomicMin of
// the first row (index0 + 64 w + lane) into first_hit[tape - result_base] and the count into
// hit_count (either may be null)
hipError_t launch_combine(const unsigned long long* masks, uint64_t stride, const uint32_t* split,
                          uint32_t n_split, uint32_t mask_base, uint32_t result_base,
                          uint64_t index0, unsigned long long* first_hit,
                          unsigned long long* hit_count, hipStream_t stream);
// the repair step (repair.hip; include/mythril_hip.h mh_repair_*).  masks[conjunct][wave] are a
// masks-mode run's (mask_base = the first conjunct tape), `stride` its sieve_mask_stride.
// fail[r] = the conjuncts row r of the run fails
hipError_t launch_fail_count(const unsigned long long* masks, uint64_t stride, uint32_t n_conj,
                             uint32_t row_count, uint32_t* fail, hipStream_t stream);
// elites[0..n_sel): the rows with the smallest (fail, row), row = row_first + r, and their picks;
// n_sel <= min(row_count, 256); one workgroup, (n_conj + 1) words of dynamic LDS
hipError_t launch_select(const unsigned long long* masks, uint64_t stride, uint32_t n_conj,
                         const uint32_t* fail, uint32_t row_first, uint32_t row_count,
                         uint32_t n_sel, uint64_t seed, mh_elite* elites, hipStream_t stream);
// rows [0, n_elites * per) of dst: the elites' src rows, children 1.. with their pick's columns
// regenerated (set_conj [g.n_sets], conj_col_off / conj_cols on the device; the caller has
// checked every index: the kernel trusts them)
hipError_t launch_mutate(const uint32_t* src, uint64_t src_stride, uint32_t* dst,
                         uint64_t dst_stride, uint32_t n_vars, const mh_elite* elites,
                         uint32_t n_elites, uint32_t per, uint32_t flags, uint64_t seed,
                         uint64_t base, const KGuide& g, const uint32_t* set_conj,
                         const uint32_t* conj_col_off, const uint32_t* conj_cols,
                         hipStream_t stream);
// hit listing (hits.hip; include/mythril_hip.h mh_run_hits).  masks[tape][wave] are a masks-mode
// run's over row_count rows (mask_base = the first tape), `stride` its sieve_mask_stride.  Per tape:
// hits[tape][0..k) = the min(k, hits) smallest satisfying rows as index0 + row of the run,
// ascending, MH_NO_HIT after them; n_hits[tape] = how many are listed; hit_count[tape] = all of them
hipError_t launch_hits_select(const unsigned long long* masks, uint64_t stride, uint32_t n_tapes,
                              uint32_t row_count, uint64_t index0, uint32_t k, uint64_t* hits,
                              uint32_t* n_hits, uint64_t* hit_count, hipStream_t stream);
// out[tape][slot][w] = column word w (column w / 8, limb w % 8) of the buffer row
// hits[tape][slot] - index_base, zero for a slot without a hit (launch_witness_rows per slot)
hipError_t launch_hits_rows(const uint32_t* assign, uint64_t stride, const uint64_t* hits,
                            uint32_t n_tapes, uint32_t k, uint64_t index_base, uint32_t n_cols,
                            uint32_t* out, hipStream_t stream);
// values[r][c][0..7] (device) into column cols[c] (device) of buffer row first + r; the caller has
// checked the columns and the row range against the buffer
hipError_t launch_scatter(uint32_t* assign, uint64_t stride, uint64_t first, uint32_t n_rows,
                          const uint32_t* cols, uint32_t n_cols, const uint32_t* values,
                          hipStream_t stream);
// One job of a batched listing round (mh_query_round_hits_many), on the device: what the three
// launches above take, per job.  masks = the job's slice of the ctx's hit masks ([tc][mask_stride],
// written by the job's masks-mode segments with mask_base = its first tape); o_* = byte offsets of
// the job's hits [tc][k] u64 / hit_count [tc] u64 / n_hits [tc] u32 / rows [tc][k][n_cols][8] u32
// in the batch's result block; sp_* = the job's spares in the uploaded block (sp_rows == 0: none).
struct HitsJob {
    const unsigned long long* masks;
    uint64_t mask_stride, index0;  // index0 = global_base: the listing's and the rows' index base
    uint32_t* assign;
    uint64_t stride;
    uint64_t o_hits, o_hit_count, o_n_hits, o_rows;
    const uint32_t* sp_cols;
    const uint32_t* sp_values;
    uint32_t row_count, k, n_cols, sp_rows, sp_n_cols, pad;
};
// The batched forms: workgroup b belongs to the job j with prefix[j] <= b < prefix[j + 1] (device
// tables of n_jobs + 1 entries; n_blocks = prefix[n_jobs]).  Select: a workgroup per (job, tape).
// Rows: one per (job, tape, slot) of the jobs with n_cols > 0.  Scatter: scatter_blocks() per job.
hipError_t launch_hits_select_batch(const HitsJob* jobs, const uint32_t* prefix, uint32_t n_jobs,
                                    uint32_t n_blocks, char* res, hipStream_t stream);
hipError_t launch_hits_rows_batch(const HitsJob* jobs, const uint32_t* prefix, uint32_t n_jobs,
                                  uint32_t n_blocks, char* res, hipStream_t stream);
hipError_t launch_scatter_batch(const HitsJob* jobs, const uint32_t* prefix, uint32_t n_jobs,
                                uint32_t n_blocks, hipStream_t stream);
uint32_t scatter_blocks(uint32_t n_rows, uint32_t n_cols);
hipError_t launch_microbench(uint32_t kind, uint32_t iters, uint32_t blocks, uint32_t* sink,
                             hipStream_t stream);

}  // namespace mh
