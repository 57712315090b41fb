// Guided candidate generator (mh_assign_generate_guided): one thread per assignment row, SoA
// writes (column v limb k of row r at word (v*8 + k)*stride + r), so a wave's 64 lanes store
// 256 contiguous bytes per limb.  The semantics are stated in include/mythril_hip.h and restated
// bit for bit in oracle/guided_gen.py; the harvest that fills the guide is
// mythril_amd/candidates.py.  Off the hot path: written once per query, before the sieve reads it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "guided_dev.h"
#include "kernels.h"

namespace {

// splitmix64 / gen_limb / limb_mask / extract_bits / base_value / chosen_alt / apply_entry:
// guided_dev.h (the repair step's mutate kernel applies the same rule, repair.hip)
using namespace mh::guided;

constexpr int kBlock = 256;

// Every column's base value written, then every set applied in order, in memory.
// (`block` = the workgroup's row block: blockIdx.x, or a batched launch's table entry)
__device__ __forceinline__ void guided_body(u32* assign, u64 stride, u64 first, u64 count,
                                            u64 seed, u64 base, const mh::KGuide& g, u32 block) {
    const u64 i = (u64)block * kBlock + threadIdx.x;
    if (i >= count) return;
    const u64 row = first + i;
    const u64 gidx = base + row;
    for (u32 v = 0; v < g.n_cols; ++v) {
        u32 val[8];
        base_value(g, v, seed, gidx, val);
        const u32 w = g.width[v];
#pragma unroll
        for (u32 k = 0; k < 8; ++k)
            assign[((u64)v * 8 + k) * stride + row] = val[k] & limb_mask(w, k);
    }
    for (u32 j = 0; j < g.n_sets; ++j) {
        const u32 alt = chosen_alt(g, j, seed, gidx);
        if (alt == ~0u) continue;
        for (u32 e = g.alt_off[alt]; e < g.alt_off[alt + 1]; ++e) apply_entry(assign, stride, row, g, e);
    }
}

// The same rows, spread over kWaves waves per 64 rows, with the leading value-only sets
// resolved in LDS: a value entry only decides which value a column ends with -- the last one
// applied, i.e. the largest entry index, since entries are laid out in set order -- so the waves
// split the sets, each lane drawing its row's alternative of a set and keeping the largest
// entry per column with an LDS atomic max ([column][row] slots); then the waves split the
// columns and write each column of each row once (the base value, or the winning entry's).  The
// sets from the first one with a copy entry on run in memory, in order, on wave 0.  The one-lane-
// per-row form stored 8 limbs per applied entry, lane-divergently, and left a 256-row launch
// four waves: 0.20 ms per launch on average, up to 0.58 (profiles/r03h).
// STAGED (round 5): the guide's set / alternative / entry-column arrays are copied into LDS
// first, so a set's chain of dependent reads (its probability and alternatives, the chosen
// alternative's entries, each entry's column) costs LDS latency instead of a global load's
// (ET-400's 256-row launch: 304 sets, 16 waves each walking 19 of them, 70 us of mostly load
// latency, profiles/r05f/pprof).
constexpr u32 kLdsRows = 64;
constexpr u32 kWaves = 16;  // a 256-row launch: 4 workgroups of 16 waves, 4 waves per SIMD
constexpr size_t kGenLds = 64 * 1024;  // LDS of one generator workgroup at most

__global__ void __launch_bounds__(kBlock)
    guided_kernel(u32* assign, u64 stride, u64 first, u64 count, u64 seed, u64 base,
                  mh::KGuide g) {
    guided_body(assign, stride, first, count, seed, base, g, blockIdx.x);
}

template <bool STAGED>
__device__ __forceinline__ void guided_lds_body(u32* assign, u64 stride, u64 first, u64 count,
                                                u64 seed, u64 base, mh::KGuide g, u32 block) {
    extern __shared__ u32 s_last[];  // [n_cols][kLdsRows]: 1 + the winning entry, 0 = none
    const u32 lane = threadIdx.x % kLdsRows, wave = threadIdx.x / kLdsRows;
    for (u32 k = threadIdx.x; k < g.n_cols * kLdsRows; k += kLdsRows * kWaves) s_last[k] = 0;
    if constexpr (STAGED) {  // the span after the last-entry slots; the pointers rebased on it
        u32* s_span = s_last + g.n_cols * kLdsRows;
        for (u32 k = threadIdx.x; k < g.span_words; k += kLdsRows * kWaves) s_span[k] = g.set_prob[k];
        g.set_off = s_span + (g.set_off - g.set_prob);
        g.alt_off = s_span + (g.alt_off - g.set_prob);
        g.entry_col = s_span + (g.entry_col - g.set_prob);
        g.set_prob = s_span;
    }
    __syncthreads();
    const u64 i = (u64)block * kLdsRows + lane;
    const bool live = i < count;
    const u64 row = first + (live ? i : 0);
    const u64 gidx = base + row;
    if (live) {
        for (u32 j = wave; j < g.n_value_sets; j += kWaves) {
            const u32 alt = chosen_alt(g, j, seed, gidx);
            if (alt == ~0u) continue;
            for (u32 e = g.alt_off[alt]; e < g.alt_off[alt + 1]; ++e)
                atomicMax(&s_last[g.entry_col[e] * kLdsRows + lane], e + 1);
        }
    }
    __syncthreads();
    if (live) {
        for (u32 v = wave; v < g.n_cols; v += kWaves) {
            const u32 e = s_last[v * kLdsRows + lane];
            u32 val[8];
            if (e == 0) {
                base_value(g, v, seed, gidx, val);
            } else {
#pragma unroll
                for (u32 k = 0; k < 8; ++k) val[k] = g.entry_val[(u64)(e - 1) * 8 + k];
            }
            const u32 w = g.width[v];
#pragma unroll
            for (u32 k = 0; k < 8; ++k)
                assign[((u64)v * 8 + k) * stride + row] = val[k] & limb_mask(w, k);
        }
    }
    if (g.n_value_sets == g.n_sets) return;
    __syncthreads();  // every column written (and visible to the workgroup) before the copies
    if (!live || wave != 0) return;
    for (u32 j = g.n_value_sets; j < g.n_sets; ++j) {
        const u32 alt = chosen_alt(g, j, seed, gidx);
        if (alt == ~0u) continue;
        for (u32 e = g.alt_off[alt]; e < g.alt_off[alt + 1]; ++e) apply_entry(assign, stride, row, g, e);
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(kLdsRows * kWaves)
    guided_lds_kernel(u32* assign, u64 stride, u64 first, u64 count, u64 seed, u64 base,
                      mh::KGuide g) {
    guided_lds_body<STAGED>(assign, stride, first, count, seed, base, g, blockIdx.x);
}

// The batched forms (mh_query_round_many): workgroup i writes row block blocks[i].block of job
// blocks[i].job, whose parameters come out of the device array `jobs` (read only) instead of the
// kernel's arguments.  Every job of a launch has the launch's form (batch_plan.h gen_form) and the
// bodies are the ones above, so a job's rows are the single-query launch's bit for bit; the
// dynamic LDS of an LDS launch is the largest any of its jobs needs.
__global__ void __launch_bounds__(kBlock)
    guided_batch_kernel(const mh::GenJob* __restrict__ jobs,
                        const mh::batch::GenEntry* __restrict__ blocks) {
    const mh::batch::GenEntry e = blocks[blockIdx.x];
    const mh::GenJob j = jobs[e.job];
    guided_body(j.assign, j.stride, 0, j.count, j.seed, j.base, j.g, e.block);
}

template <bool STAGED>
__global__ void __launch_bounds__(kLdsRows * kWaves)
    guided_lds_batch_kernel(const mh::GenJob* __restrict__ jobs,
                            const mh::batch::GenEntry* __restrict__ blocks) {
    const mh::batch::GenEntry e = blocks[blockIdx.x];
    const mh::GenJob j = jobs[e.job];
    guided_lds_body<STAGED>(j.assign, j.stride, 0, j.count, j.seed, j.base, j.g, e.block);
}

__global__ void __launch_bounds__(kBlock)
    results_reset_kernel(u64* first_hit, u64* hit_count, u32 n) {
    const u32 i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (first_hit) first_hit[i] = ~0ull;
    if (hit_count) hit_count[i] = 0;
}

// one workgroup per tape: the words of its witness row (a row outside the buffer reads as none)
__global__ void __launch_bounds__(kBlock)
    witness_rows_kernel(const u32* assign, u64 stride, const u64* first_hit, u64 index_base,
                        u32 n_cols, u32* out) {
    const u64 h = first_hit[blockIdx.x];
    const u64 row = h - index_base;
    const bool hit = h != ~0ull && h >= index_base && row < stride;
    const u32 words = n_cols * 8;
    u32* o = out + (u64)blockIdx.x * words;
    for (u32 w = threadIdx.x; w < words; w += kBlock) o[w] = hit ? assign[(u64)w * stride + row] : 0u;
}

// the batched reset and gather over the jobs' slices of one result block (kernels.h ResultJob)
__global__ void __launch_bounds__(kBlock) results_reset_batch_kernel(const mh::ResultJob* jobs) {
    const mh::ResultJob j = jobs[blockIdx.x];
    for (u32 i = threadIdx.x; i < j.tc; i += kBlock) {
        j.first_hit[i] = ~0ull;
        j.first_hit[j.tc + i] = 0;
    }
}

__global__ void __launch_bounds__(kBlock) witness_rows_batch_kernel(const mh::ResultJob* jobs) {
    const mh::ResultJob j = jobs[blockIdx.y];
    const u32 words = j.n_cols * 8;
    u32* rows = reinterpret_cast<u32*>(j.first_hit + 2 * (u64)j.tc);
    for (u32 t = blockIdx.x; t < j.tc; t += gridDim.x) {
        const u64 h = j.first_hit[t];
        const u64 row = h - j.index_base;
        const bool hit = h != ~0ull && h >= j.index_base && row < j.stride;
        u32* o = rows + (u64)t * words;
        for (u32 w = threadIdx.x; w < words; w += kBlock)
            o[w] = hit ? j.assign[(u64)w * j.stride + row] : 0u;
    }
}

}  // namespace

namespace mh {

hipError_t launch_generate_guided_batch(const GenJob* jobs, const batch::GenEntry* blocks,
                                        uint32_t n_blocks, uint32_t form, uint64_t lds_bytes,
                                        hipStream_t stream) {
    if (n_blocks == 0) return hipSuccess;
    if (lds_bytes > kGenLds) return hipErrorInvalidValue;
    if (form == batch::kFormStaged)
        hipLaunchKernelGGL(guided_lds_batch_kernel<true>, dim3(n_blocks), dim3(kLdsRows * kWaves),
                           (size_t)lds_bytes, stream, jobs, blocks);
    else if (form == batch::kFormLds)
        hipLaunchKernelGGL(guided_lds_batch_kernel<false>, dim3(n_blocks), dim3(kLdsRows * kWaves),
                           (size_t)lds_bytes, stream, jobs, blocks);
    else if (form == batch::kFormMem)
        hipLaunchKernelGGL(guided_batch_kernel, dim3(n_blocks), dim3(kBlock), 0, stream, jobs,
                           blocks);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_results_reset_batch(const ResultJob* jobs, uint32_t n_jobs, hipStream_t stream) {
    if (n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(results_reset_batch_kernel, dim3(n_jobs), dim3(kBlock), 0, stream, jobs);
    return hipGetLastError();
}

hipError_t launch_witness_rows_batch(const ResultJob* jobs, uint32_t n_jobs, uint32_t max_tc,
                                     hipStream_t stream) {
    if (n_jobs == 0 || max_tc == 0) return hipSuccess;
    hipLaunchKernelGGL(witness_rows_batch_kernel, dim3(std::min<uint32_t>(max_tc, 16), n_jobs),
                       dim3(kBlock), 0, stream, jobs);
    return hipGetLastError();
}

hipError_t launch_results_reset(uint64_t* first_hit, uint64_t* hit_count, uint32_t n,
                                hipStream_t stream) {
    if (n == 0 || (!first_hit && !hit_count)) return hipSuccess;
    hipLaunchKernelGGL(results_reset_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                       first_hit, hit_count, n);
    return hipGetLastError();
}

hipError_t launch_witness_rows(const uint32_t* assign, uint64_t stride, const uint64_t* first_hit,
                               uint32_t n_tapes, uint64_t index_base, uint32_t n_cols,
                               uint32_t* out, hipStream_t stream) {
    if (n_tapes == 0 || n_cols == 0) return hipSuccess;
    hipLaunchKernelGGL(witness_rows_kernel, dim3(n_tapes), dim3(kBlock), 0, stream, assign, stride,
                       first_hit, index_base, n_cols, out);
    return hipGetLastError();
}

hipError_t launch_generate_guided(uint32_t* assign, uint64_t stride, uint64_t first,
                                  uint64_t count, uint64_t seed, uint64_t base, const KGuide& g,
                                  hipStream_t stream) {
    if (count == 0) return hipSuccess;
    // LDS form while the last-entry slots (256 B per column) fit 48 KB per workgroup
    // (batch_plan.h gen_form: the rule the batched launches pick a job's form by)
    const size_t lds = (size_t)mh::batch::gen_lds_bytes(g.n_cols);
    const size_t staged = (size_t)mh::batch::gen_staged_bytes(g.n_cols, g.span_words);
    const u64 blocks = (count + kLdsRows - 1) / kLdsRows;
    const mh::batch::GenForm form = mh::batch::gen_form(g.n_cols, g.span_words);
    if (form == mh::batch::kFormStaged) {
        hipLaunchKernelGGL(guided_lds_kernel<true>, dim3((unsigned)blocks), dim3(kLdsRows * kWaves),
                           staged, stream, assign, stride, first, count, seed, base, g);
    } else if (form == mh::batch::kFormLds) {
        hipLaunchKernelGGL(guided_lds_kernel<false>, dim3((unsigned)blocks), dim3(kLdsRows * kWaves),
                           lds, stream, assign, stride, first, count, seed, base, g);
    } else {
        const u64 blocks = (count + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(guided_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, assign,
                           stride, first, count, seed, base, g);
    }
    return hipGetLastError();
}

}  // namespace mh
