// TEST-ONLY host emulator of the interpreter with register spilling (not part of libmythril_hip).
//
// tests/native/emu.cpp compiles tapes the way every caller without spill hooks does: a tape that
// runs out of registers is refused.  This one asks the tape compiler for the spilling attempt
// (compile_tape's allow_spill, what mh_tapes_compile does) and runs the instruction stream
// through exec.h's step() with F_SPILL and a machine that has the spill() / fill() hooks: a slot
// array per row, where the device keeps an area per wave.  tests/test_spill_host.py checks the
// allocator's spill code and the two ops against the Python oracle with it, without a GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "compile.h"
#include "exec.h"
#include "u256_ops.h"

using namespace mh;

namespace {

struct SpillMachine {
    u32 R[MH_NR_MAX + 1][8];
    u32 nrx_;
    const u32* slots;  // the tape's slot words (w0, w1 pairs)
    const u32* assign;
    u64 cap, row;
    u32* spills;  // this row's spill slots, 8 limbs each
    u32 nrx() const { return nrx_; }
    void read(u32 r, u32* v) const { memcpy(v, R[r], 32); }
    u32 read0(u32 r) const { return R[r][0]; }
    void write(u32 r, const u32* v) { memcpy(R[r], v, 32); }
    void iconst(u32 slot, u32* v) const { memcpy(v, slots + 2ull * slot, 32); }
    void var(u32 col, u32* v) const {
        for (int k = 0; k < 8; ++k) v[k] = assign[((u64)col * 8 + k) * cap + row];
    }
    void spill(u32 slot, const u32* v) { memcpy(spills + 8ull * slot, v, 32); }
    void fill(u32 slot, u32* v) const { memcpy(v, spills + 8ull * slot, 32); }
};

// every tape of the set, as mh_tapes_compile compiles it; `sel` gets tape `tape`'s summary and
// its first slot
int32_t compile_all(const mh_node* nodes, const uint64_t* offs, uint32_t n_tapes,
                    const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                    std::vector<uint32_t>& words, std::vector<CompiledTape>& cts,
                    std::vector<uint32_t>& first, char* err, int errlen) {
    std::vector<uint32_t> dconsts;
    mh::ConstIndex dindex;
    for (uint32_t t = 0; t < n_tapes; ++t) {
        CompiledTape ct;
        std::string e;
        first.push_back((uint32_t)(words.size() / 2));
        const int32_t r = compile_tape(nodes + offs[t], (size_t)(offs[t + 1] - offs[t]), consts,
                                       n_consts, n_vars, dconsts, dindex, words, ct, e, true);
        if (r != MH_OK) {
            snprintf(err, errlen, "tape %u: %s", t, e.c_str());
            return r;
        }
        if (((ct.features & F_SPILL) != 0) != (ct.n_spills > 0)) {
            snprintf(err, errlen, "tape %u: F_SPILL and the slot count disagree", t);
            return MH_E_INVALID;
        }
        cts.push_back(ct);
    }
    return MH_OK;
}

}  // namespace

// Root values of tape `tape` over `rows` rows of `assign` ([n_vars][8][rows]): out[k * rows + row].
extern "C" int32_t spill_emu_eval(const mh_node* nodes, const uint64_t* offs, uint32_t n_tapes,
                                  const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                                  uint32_t tape, const uint32_t* assign, uint64_t rows,
                                  uint32_t* out, uint32_t* n_regs_out, char* err, int errlen) {
    std::vector<uint32_t> words, first;
    std::vector<CompiledTape> cts;
    if (int32_t r = compile_all(nodes, offs, n_tapes, consts, n_consts, n_vars, words, cts, first,
                                err, errlen))
        return r;
    if (tape >= n_tapes) return MH_E_INVALID;
    const CompiledTape sel = cts[tape];
    if (n_regs_out) *n_regs_out = sel.n_regs;
    const uint32_t n_pre = n_vars <= MH_MAX_PRELOAD ? n_vars : 0;
    const u32* ip = words.data() + 2ull * first[tape];
    const u32 nrx = mh_nrx_of(sel.n_regs);
    std::vector<u32> spills(8ull * sel.n_spills + 8);
    for (uint64_t row = 0; row < rows; ++row) {
        SpillMachine m;
        memset(m.R, 0xCD, sizeof(m.R));  // poison: reads of never-written registers show up
        memset(spills.data(), 0xCD, spills.size() * 4);
        m.nrx_ = nrx;
        m.slots = ip;
        m.assign = assign;
        m.cap = rows;
        m.row = row;
        m.spills = spills.data();
        for (uint32_t v = 0; v < n_pre; ++v)
            for (int k = 0; k < 8; ++k) m.R[v][k] = assign[((u64)v * 8 + k) * rows + row];
        u32 s = 0;
        for (;;) {
            if (s >= sel.n_insns) {
                snprintf(err, errlen, "tape ran past its slots");
                return MH_E_INVALID;
            }
            const u32 w0 = ip[2 * s], w1 = ip[2 * s + 1];
            const u32 op = w1 & 0xFFu;
            if (op == D_END) break;
            if (op == D_WINDOW) {
                s = (s / MH_WINDOW + 1) * MH_WINDOW;
                continue;
            }
            if ((op == D_SPILL || op == D_FILL) && ((w1 >> 17) & MH_AUX_MAX) >= sel.n_spills) {
                snprintf(err, errlen, "spill slot beyond the tape's %u at slot %u", sel.n_spills, s);
                return MH_E_INVALID;
            }
            s += step<F_DIV | F_KECCAK | F_EVM | F_SPILL, true>(m, w0, w1, s);
            // the device leaves the tape at a D_BANDZ whose conjunction is 0 in every lane of a
            // wave; here in the lane alone (stricter: the root must then be 0 for this row)
            if (op == D_BANDZ && (m.R[nrx][0] & 1u) == 0) break;
            if (mh_produces_bool(op) && m.R[nrx][0] > 1u) {
                snprintf(err, errlen, "non-canonical Bool from op %u at slot %u", op, s);
                return MH_E_INVALID;
            }
        }
        u32 res[8];
        memcpy(res, m.R[nrx], 32);
        if (sel.root_bool) {
            res[0] &= 1u;
            for (int k = 1; k < 8; ++k) res[k] = 0;
        }
        for (int k = 0; k < 8; ++k) out[(u64)k * rows + row] = res[k];
    }
    return MH_OK;
}

// The concatenated slot words of every tape; *n_words_out = the u32 words needed, copied when
// they fit in cap.
extern "C" int32_t spill_emu_words(const mh_node* nodes, const uint64_t* offs, uint32_t n_tapes,
                                   const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                                   uint32_t* out, uint64_t cap, uint64_t* n_words_out, char* err,
                                   int errlen) {
    std::vector<uint32_t> words, first;
    std::vector<CompiledTape> cts;
    if (int32_t r = compile_all(nodes, offs, n_tapes, consts, n_consts, n_vars, words, cts, first,
                                err, errlen))
        return r;
    *n_words_out = words.size();
    if (words.size() <= cap) memcpy(out, words.data(), words.size() * 4);
    return MH_OK;
}

// Spill slots per tape (the library's mh_tapes_spills).
extern "C" int32_t spill_emu_tape_spills(const mh_node* nodes, const uint64_t* offs,
                                         uint32_t n_tapes, const uint32_t* consts,
                                         uint32_t n_consts, uint32_t n_vars, uint32_t* out,
                                         char* err, int errlen) {
    std::vector<uint32_t> words, first;
    std::vector<CompiledTape> cts;
    if (int32_t r = compile_all(nodes, offs, n_tapes, consts, n_consts, n_vars, words, cts, first,
                                err, errlen))
        return r;
    for (uint32_t t = 0; t < n_tapes; ++t) out[t] = cts[t].n_spills;
    return MH_OK;
}
