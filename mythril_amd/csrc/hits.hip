// Hit listing (include/mythril_hip.h mh_run_hits / mh_assign_scatter; DESIGN.md §6 "Spare
// witnesses"): the kernels after the interpreter has written one 64-row Bool mask per (tape, wave
// of the run) -- KParams::masks, the masks the repair step scores.
//   hits_select_kernel  masks[tape][wave] -> the k smallest satisfying rows of every tape, ascending,
//                       as global indices; how many were listed; the tape's whole hit count
//   hits_rows_kernel    the first n_cols columns of every listed row
//   scatter_kernel      host-given values into chosen columns of a run of buffer rows
// and their batched forms (mh_query_round_hits_many): the same bodies, a job's arguments out of a
// device table, so a job's list cannot differ from the single call's.
// Restated in tests/hits_ref.py.  Nothing here runs unless Sieve(spares > 0) or a caller of the
// three entry points asks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace {

using u32 = uint32_t;
using u64 = uint64_t;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr u64 kNoHit = ~0ull;  // MH_NO_HIT

// One workgroup per tape.  The mask words are walked in row order, 256 words (16384 rows) at a time,
// one word per thread; a block-wide exclusive prefix sum of the words' popcounts gives every word
// the slot of its first set bit, so the list is in row order whatever the scheduling.  Placing
// stops once k slots are filled; the words after that are only counted.  Integer only.  Bits at or
// past row_count in the last word are masked off here (nothing else pins them).
// (the body of both select kernels: m_t = the tape's mask words, out = its k list slots)
__device__ __forceinline__ void select_tape(const unsigned long long* m_t, u32 row_count, u64 index0,
                                            u32 k, u64* out, u32* n_hits_t, u64* hit_count_t) {
    __shared__ u32 s_wave[kWaves];
    __shared__ u32 s_run;    // hits in the words walked so far
    __shared__ u32 s_total;  // the tape's hits
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 n_words = (row_count + 63u) >> 6;
    const u32 tail = row_count & 63u;
    if (tid == 0) {
        s_run = 0;
        s_total = 0;
    }
    __syncthreads();
    u32 mine = 0;  // popcount of this thread's words
    u32 c0 = 0;
    for (; c0 < n_words; c0 += kBlock) {
        const u32 w = c0 + tid;
        unsigned long long m = w < n_words ? m_t[w] : 0ull;
        if (tail && w == n_words - 1) m &= (1ull << tail) - 1ull;
        const u32 pc = (u32)__builtin_popcountll(m);
        mine += pc;
        u32 incl = pc;  // inclusive scan over the wave
#pragma unroll
        for (u32 d = 1; d < 64; d <<= 1) {
            const u32 v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        u32 slot = s_run + incl - pc;
        for (u32 i = 0; i < wave; ++i) slot += s_wave[i];
        while (m && slot < k) {
            out[slot++] = index0 + (u64)w * 64u + (u64)__builtin_ctzll(m);
            m &= m - 1ull;
        }
        __syncthreads();
        if (tid == 0) {
            u32 sum = 0;
            for (u32 i = 0; i < (u32)kWaves; ++i) sum += s_wave[i];
            s_run += sum;
        }
        __syncthreads();
        if (s_run >= k) {  // uniform: read after the barrier
            c0 += kBlock;
            break;
        }
    }
    for (; c0 < n_words; c0 += kBlock) {  // k are placed: the rest is counted only
        const u32 w = c0 + tid;
        unsigned long long m = w < n_words ? m_t[w] : 0ull;
        if (tail && w == n_words - 1) m &= (1ull << tail) - 1ull;
        mine += (u32)__builtin_popcountll(m);
    }
    if (mine) atomicAdd(&s_total, mine);  // a sum: the order does not matter
    __syncthreads();
    const u32 total = s_total, n = total < k ? total : k;
    for (u32 j = n + tid; j < k; j += kBlock) out[j] = kNoHit;
    if (tid == 0) {
        *n_hits_t = n;
        *hit_count_t = total;
    }
}

__global__ void __launch_bounds__(kBlock)
    hits_select_kernel(const unsigned long long* masks, u64 stride, u32 row_count, u64 index0, u32 k,
                       u64* hits, u32* n_hits, u64* hit_count) {
    const u32 t = blockIdx.x;
    select_tape(masks + (u64)t * stride, row_count, index0, k, hits + (u64)t * k, n_hits + t,
                hit_count + t);
}

// The batched forms (mh_query_round_hits_many): the same bodies per job, the job's arguments read
// from its HitsJob (kernels.h).  prefix[j] = the workgroups of the jobs before job j, prefix[n_jobs]
// = the grid: a workgroup finds its job by bisection (a job may own none), at a wave-uniform
// address, so the loads are scalar.
__device__ __forceinline__ u32 job_of(const u32* prefix, u32 n_jobs, u32 b) {
    u32 lo = 0, hi = n_jobs;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (prefix[mid + 1] <= b) lo = mid + 1;
        else hi = mid;
    }
    return lo;  // prefix[lo] <= b < prefix[lo + 1]
}

// one workgroup per (job, tape)
__global__ void __launch_bounds__(kBlock)
    hits_select_batch_kernel(const mh::HitsJob* jobs, const u32* prefix, u32 n_jobs, char* res) {
    const u32 ji = job_of(prefix, n_jobs, blockIdx.x);
    const mh::HitsJob j = jobs[ji];
    const u32 t = blockIdx.x - prefix[ji];
    select_tape(j.masks + (u64)t * j.mask_stride, j.row_count, j.index0, j.k,
                reinterpret_cast<u64*>(res + j.o_hits) + (u64)t * j.k,
                reinterpret_cast<u32*>(res + j.o_n_hits) + t,
                reinterpret_cast<u64*>(res + j.o_hit_count) + t);
}

// one workgroup per (tape, slot): out[tape][slot][w] = column word w of the buffer row the slot
// lists, zero for a slot without a hit (a row outside the buffer reads as none, as in
// witness_rows_kernel)
__device__ __forceinline__ void rows_slot(const u32* assign, u64 stride, const u64* hits,
                                          u64 index_base, u32 n_cols, u32* out, u64 s) {
    const u64 h = hits[s];
    const u64 row = h - index_base;
    const bool hit = h != kNoHit && h >= index_base && row < stride;
    const u32 words = n_cols * 8;
    u32* o = out + s * words;
    for (u32 w = threadIdx.x; w < words; w += kBlock) o[w] = hit ? assign[(u64)w * stride + row] : 0u;
}

__global__ void __launch_bounds__(kBlock)
    hits_rows_kernel(const u32* assign, u64 stride, const u64* hits, u64 index_base,
                     u32 n_cols, u32* out) {
    rows_slot(assign, stride, hits, index_base, n_cols, out, blockIdx.x);  // tape * k + slot
}

// one workgroup per (job, tape, slot) of the jobs that ask for rows
__global__ void __launch_bounds__(kBlock)
    hits_rows_batch_kernel(const mh::HitsJob* jobs, const u32* prefix, u32 n_jobs, char* res) {
    const u32 ji = job_of(prefix, n_jobs, blockIdx.x);
    const mh::HitsJob j = jobs[ji];
    rows_slot(j.assign, j.stride, reinterpret_cast<const u64*>(res + j.o_hits), j.index0, j.n_cols,
              reinterpret_cast<u32*>(res + j.o_rows), blockIdx.x - prefix[ji]);
}

// one thread per (column, limb, row), the row fastest: values[r][c][l] -> column cols[c], limb l of
// buffer row first + r
__device__ __forceinline__ void scatter_word(u32* assign, u64 stride, u64 first, u32 n_rows,
                                             const u32* cols, u32 n_cols, const u32* values,
                                             u64 i) {
    if (i >= (u64)n_rows * n_cols * 8) return;
    const u32 r = (u32)(i % n_rows), cl = (u32)(i / n_rows), c = cl >> 3, l = cl & 7u;
    assign[((u64)cols[c] * 8 + l) * stride + first + r] = values[((u64)r * n_cols + c) * 8 + l];
}

__global__ void __launch_bounds__(kBlock)
    scatter_kernel(u32* assign, u64 stride, u64 first, u32 n_rows, const u32* cols, u32 n_cols,
                   const u32* values) {
    scatter_word(assign, stride, first, n_rows, cols, n_cols, values,
                 (u64)blockIdx.x * kBlock + threadIdx.x);
}

// every job's spares into rows [0, sp_rows) of its buffer: prefix counts kBlock-thread workgroups
__global__ void __launch_bounds__(kBlock)
    scatter_batch_kernel(const mh::HitsJob* jobs, const u32* prefix, u32 n_jobs) {
    const u32 ji = job_of(prefix, n_jobs, blockIdx.x);
    const mh::HitsJob j = jobs[ji];
    scatter_word(j.assign, j.stride, 0, j.sp_rows, j.sp_cols, j.sp_n_cols, j.sp_values,
                 (u64)(blockIdx.x - prefix[ji]) * kBlock + threadIdx.x);
}

}  // namespace

namespace mh {

hipError_t launch_hits_select(const unsigned long long* masks, uint64_t stride, uint32_t n_tapes,
                              uint32_t row_count, uint64_t index0, uint32_t k, uint64_t* hits,
                              uint32_t* n_hits, uint64_t* hit_count, hipStream_t stream) {
    if (n_tapes == 0) return hipSuccess;
    if (k == 0 || row_count == 0 || ((uint64_t)row_count + 63) / 64 > stride)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hits_select_kernel, dim3(n_tapes), dim3(kBlock), 0, stream, masks, stride,
                       row_count, index0, k, hits, n_hits, hit_count);
    return hipGetLastError();
}

hipError_t launch_hits_rows(const uint32_t* assign, uint64_t stride, const uint64_t* hits,
                            uint32_t n_tapes, uint32_t k, uint64_t index_base, uint32_t n_cols,
                            uint32_t* out, hipStream_t stream) {
    if (n_tapes == 0 || n_cols == 0 || k == 0) return hipSuccess;
    if ((uint64_t)n_tapes * k > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hits_rows_kernel, dim3(n_tapes * k), dim3(kBlock), 0, stream, assign, stride,
                       hits, index_base, n_cols, out);
    return hipGetLastError();
}

hipError_t launch_scatter(uint32_t* assign, uint64_t stride, uint64_t first, uint32_t n_rows,
                          const uint32_t* cols, uint32_t n_cols, const uint32_t* values,
                          hipStream_t stream) {
    const uint64_t n = (uint64_t)n_rows * n_cols * 8;
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, assign,
                       stride, first, n_rows, cols, n_cols, values);
    return hipGetLastError();
}

hipError_t launch_hits_select_batch(const HitsJob* jobs, const uint32_t* prefix, uint32_t n_jobs,
                                    uint32_t n_blocks, char* res, hipStream_t stream) {
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(hits_select_batch_kernel, dim3(n_blocks), dim3(kBlock), 0, stream, jobs,
                       prefix, n_jobs, res);
    return hipGetLastError();
}

hipError_t launch_hits_rows_batch(const HitsJob* jobs, const uint32_t* prefix, uint32_t n_jobs,
                                  uint32_t n_blocks, char* res, hipStream_t stream) {
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(hits_rows_batch_kernel, dim3(n_blocks), dim3(kBlock), 0, stream, jobs, prefix,
                       n_jobs, res);
    return hipGetLastError();
}

hipError_t launch_scatter_batch(const HitsJob* jobs, const uint32_t* prefix, uint32_t n_jobs,
                                uint32_t n_blocks, hipStream_t stream) {
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_batch_kernel, dim3(n_blocks), dim3(kBlock), 0, stream, jobs, prefix,
                       n_jobs);
    return hipGetLastError();
}

uint32_t scatter_blocks(uint32_t n_rows, uint32_t n_cols) {
    return (uint32_t)(((uint64_t)n_rows * n_cols * 8 + kBlock - 1) / kBlock);
}

}  // namespace mh
