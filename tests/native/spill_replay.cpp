// Replays a corpus of one-tape sets (tests/test_spill_host.py: the fan tapes and the fuzz tapes of
// tests/spill_cases.py) through the tape compiler's interpreter lowering, spilling allocation
// included (csrc/compile.cpp), and the host emulator (spill_emu.cpp: exec.h's step() with the spill /
// fill hooks), all built into this executable for AddressSanitizer / UBSan runs (test
// infrastructure, no device).  Every slot count and output word must equal the corpus's (the
// unsanitized build's).
//
// Format (little-endian): u32 n_sets, then per set: u32 n_vars, n_consts, rows, n_nodes,
// mh_node nodes[n_nodes], u32 consts[n_consts][8], u32 soa[n_vars][8][rows], u32 spill slots,
// u32 values[8][rows].
//
//   spill_replay CORPUS     -> prints "sets=S spilled=M", exit 0
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mythril_hip.h"

extern "C" int32_t spill_emu_eval(const mh_node* nodes, const uint64_t* offs, uint32_t n_tapes,
                            const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                            uint32_t tape, const uint32_t* assign, uint64_t rows, uint32_t* out,
                            uint32_t* n_regs_out, char* err, int errlen);
extern "C" int32_t spill_emu_tape_spills(const mh_node* nodes, const uint64_t* offs, uint32_t n_tapes,
                                   const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                                   uint32_t* out, char* err, int errlen);

namespace {

struct In {
    FILE* f;
    bool ok = true;
    uint32_t u32() {
        uint32_t v = 0;
        ok = ok && std::fread(&v, sizeof v, 1, f) == 1;
        return v;
    }
    template <class T>
    std::vector<T> arr(size_t n) {
        std::vector<T> v(n ? n : 1);
        ok = ok && (n == 0 || std::fread(v.data(), sizeof(T), n, f) == n);
        return v;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: spill_replay CORPUS\n");
        return 2;
    }
    In in{std::fopen(argv[1], "rb")};
    if (!in.f) { std::perror("open"); return 2; }
    const uint32_t n_sets = in.u32();
    uint32_t spilled = 0;
    char err[512];
    for (uint32_t s = 0; s < n_sets && in.ok; ++s) {
        const uint32_t n_vars = in.u32(), n_consts = in.u32(), rows = in.u32(), n_nodes = in.u32();
        auto nodes = in.arr<mh_node>(n_nodes);
        auto consts = in.arr<uint32_t>(8ull * n_consts);
        auto soa = in.arr<uint32_t>(8ull * n_vars * rows);
        const uint32_t want_slots = in.u32();
        auto want = in.arr<uint32_t>(8ull * rows);
        if (!in.ok) { std::fprintf(stderr, "truncated corpus\n"); return 2; }
        const uint64_t offs[2] = {0, n_nodes};
        uint32_t slots = 0;
        int32_t r = spill_emu_tape_spills(nodes.data(), offs, 1, consts.data(), n_consts, n_vars, &slots,
                                    err, sizeof err);
        if (r != 0 || slots != want_slots) {
            std::fprintf(stderr, "set %u: %u spill slots, corpus %u (rc %d %s)\n", s, slots,
                         want_slots, r, r ? err : "");
            return 1;
        }
        std::vector<uint32_t> out(8ull * rows);
        uint32_t n_regs = 0;
        r = spill_emu_eval(nodes.data(), offs, 1, consts.data(), n_consts, n_vars, 0, soa.data(), rows,
                     out.data(), &n_regs, err, sizeof err);
        if (r != 0 || out != std::vector<uint32_t>(want.begin(), want.begin() + out.size())) {
            std::fprintf(stderr, "set %u: values differ (rc %d %s)\n", s, r, r ? err : "");
            return 1;
        }
        spilled += slots != 0;
    }
    std::fclose(in.f);
    if (!in.ok) { std::fprintf(stderr, "truncated corpus\n"); return 2; }
    std::printf("sets=%u spilled=%u\n", n_sets, spilled);
    return 0;
}
