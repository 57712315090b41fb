// Enumerating generator (mh_assign_enumerate): the cross product of a group's finite domains
// written in order, one thread per assignment row, SoA writes as generate.hip's (column v limb k
// of row r at word (v*8 + k)*stride + r, so a wave's 64 lanes store 256 contiguous bytes per
// limb).  The semantics are stated in include/mythril_hip.h and restated bit for bit in
// mythril_amd/decide.py enumerate_rows.  The descriptors are read-only and the same for every
// lane, so the loop over the columns is wave-uniform; only the digit differs per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace {

constexpr int kBlock = 256;

// Row first + i gets global index g = base + i.  The digit of column j is (g / stride_j) mod
// size_j with stride_j the product of the earlier sizes: the running quotient q_j = g / stride_j
// (q_0 = g, q_{j+1} = q_j / size_j) gives the same number without the strides, stays exact when
// their product passes 2^64 (q is 0 from there on: digit 0), and needs one division per column,
// a 32-bit one once the quotient and the size fit.
__global__ void __launch_bounds__(kBlock)
    enumerate_kernel(uint32_t* assign, uint64_t stride, uint64_t first, uint64_t count,
                     uint64_t base, const mh::KDomain* __restrict__ doms, uint32_t n_doms,
                     const uint32_t* __restrict__ list_vals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint64_t row = first + i;
    uint64_t q = base + i;
    for (uint32_t j = 0; j < n_doms; ++j) {
        const mh::KDomain& dm = doms[j];
        const uint64_t size = dm.size;
        uint64_t d = 0;
        if (q != 0) {
            if (((q | size) >> 32) == 0) {
                d = (uint32_t)q % (uint32_t)size;
                q = (uint32_t)q / (uint32_t)size;
            } else {
                d = q % size;
                q = q / size;
            }
        }
        uint32_t val[8];
        if (dm.kind == MH_DOMAIN_LIST) {
            const uint32_t* v = list_vals + ((uint64_t)dm.list_off + d) * 8;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) val[k] = v[k];
        } else {  // lo + d: the carry crosses every limb
            uint64_t s = (uint64_t)dm.lo[0] + (uint32_t)d;
            val[0] = (uint32_t)s;
            s = (uint64_t)dm.lo[1] + (uint32_t)(d >> 32) + (s >> 32);
            val[1] = (uint32_t)s;
#pragma unroll
            for (uint32_t k = 2; k < 8; ++k) {
                s = (uint64_t)dm.lo[k] + (s >> 32);
                val[k] = (uint32_t)s;
            }
        }
        uint32_t* out = assign + (uint64_t)dm.col * 8 * stride + row;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) out[(uint64_t)k * stride] = val[k];
    }
}

}  // namespace

namespace mh {

hipError_t launch_enumerate(uint32_t* assign, uint64_t stride, uint64_t first, uint64_t count,
                            uint64_t base, const KDomain* doms, uint32_t n_doms,
                            const uint32_t* list_vals, hipStream_t stream) {
    if (count == 0 || n_doms == 0) return hipSuccess;
    const uint64_t blocks = (count + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(enumerate_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, assign,
                       stride, first, count, base, doms, n_doms, list_vals);
    return hipGetLastError();
}

}  // namespace mh
