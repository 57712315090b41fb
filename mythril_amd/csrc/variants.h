// The interpreter's kernel variants: which kernel a tape runs in, which buffers a variant can
// address, and what a launch of the spill variant needs of spill memory.  Host-only numbers (no HIP
// header), shared by the launch interface (kernels.h), the planners (launch_plan.h, batch_plan.h,
// values_plan.h) and their stand-alone checks under tests/native.
#pragma once
#include <stdint.h>

#include "dev_isa.h"

namespace mh {

// Kernel variants: register-file size class (NR 7 / 9 / 15) x feature set (asm only / + C++
// complex ops / + keccak / + keccak and the EVM helpers).  Keccak tapes get a kernel without the
// EVM helpers' register footprint.
inline uint32_t nr_class(uint32_t n_regs) {
    return n_regs <= MH_NR_SMALL ? 0u : n_regs <= MH_NR_MID ? 1u : 2u;
}
// A register class's variants are consecutive: class c is [c * kClassVariants, (c + 1) *
// kClassVariants), feature sets nesting upwards inside it (a kernel with more handlers runs a tape
// that needs fewer).
constexpr uint32_t kClassVariants = 4;
// Tapes with a table lookup (F_TABLE: the certifier's, never a query round's) get a feature class
// of their own with every handler, one kernel per register class, numbered after the twelve.
constexpr uint32_t kFirstTableVariant = 12;
// Tapes that spill (F_SPILL: more live values than MH_NR_MAX registers, compile.cpp) run in one
// kernel of their own, NR = 15 with every handler, the table lookup included, and the spill ops:
// no other variant carries a case, a branch or a register for them.
constexpr uint32_t kSpillVariant = 15;
constexpr uint32_t kNumVariants = 16;
// the three register classes, then a fourth of the table variants and the spill variant
constexpr uint32_t kNumClasses = kNumVariants / kClassVariants;
inline uint32_t variant_of(uint32_t n_regs, uint32_t features) {
    if (features & F_SPILL) return kSpillVariant;
    if (features & F_TABLE) return kFirstTableVariant + nr_class(n_regs);  // 12..14
    const uint32_t fc = (features & F_EVM) ? 3u : (features & F_KECCAK) ? 2u
                        : (features & F_CPLX) ? 1u : 0u;
    return nr_class(n_regs) * kClassVariants + fc;  // 0..11
}
// The complex-op variants (feature class != 0) load columns inside the asm core (run_lv) with a
// 32-bit byte stride per limb plane: their buffers hold fewer than 2^30 rows per column.  The
// asm-only variants index columns with 64-bit arithmetic and take any capacity.
constexpr uint64_t kLoadvarMaxCapacity = 1ull << 30;
inline bool variant_fits(uint32_t variant, uint64_t capacity) {
    return (variant < kFirstTableVariant && (variant & 3u) == 0) || capacity < kLoadvarMaxCapacity;
}
// words of spill memory a launch of `waves` waves needs (kernels.h KParams::spill)
inline uint64_t spill_words(uint64_t waves, uint32_t spill_slots) {
    return waves * spill_slots * MH_SPILL_SLOT_WORDS;
}

}  // namespace mh
