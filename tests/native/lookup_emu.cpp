// TEST-ONLY host emulator of the interpreter with a table set (not part of libmythril_hip).
//
// tests/native/emu.cpp's machine has no tables and instantiates step() without F_TABLE; this one
// has them: it validates and packs the caller's tables with the library's own pack_tables()
// (mythril_amd/csrc/compile.cpp, what mh_tables_create runs), compiles the tape with the tape
// compiler and runs the instruction stream through exec.h's step<... | F_TABLE, true>, the code
// the device's table variants run for D_LOOKUP.  tests/test_certify.py loads it as a shared
// library; built with -DLOOKUP_EMU_MAIN it is a stand-alone program (its own main) that drives
// the table validation and the LOOKUP compile path, for a sanitizer build run directly.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "compile.h"
#include "exec.h"
#include "u256_ops.h"

using namespace mh;

struct TableMachine {
    u32 R[MH_NR_MAX + 1][8];
    u32 nrx_;
    const u32* slots;
    const u32* assign;
    u64 cap, row;
    const u32* tables;
    u32 nrx() const { return nrx_; }
    void read(u32 r, u32* v) const { memcpy(v, R[r], 32); }
    u32 read0(u32 r) const { return R[r][0]; }
    void write(u32 r, const u32* v) { memcpy(R[r], v, 32); }
    void iconst(u32 slot, u32* v) const { memcpy(v, slots + 2ull * slot, 32); }
    void var(u32 col, u32* v) const {
        for (int k = 0; k < 8; ++k) v[k] = assign[((u64)col * 8 + k) * cap + row];
    }
    void lookup(u32 table, u32 nw, const u32* k0, const u32* k1, const u32* k2, u32 hit,
                u32* z) const {
        table_lookup(tables, table, nw, k0, k1, k2, hit, z);
    }
};

// Root values of tape `tape` for `rows` rows of `assign` ([n_vars][8][rows]) over the tables:
// out[k * rows + row].  Returns pack_tables' / compile_tape's code on a refusal, `err` set.
extern "C" int32_t lookup_emu_eval(const mh_node* nodes, const uint64_t* offs, uint32_t n_tapes,
                                   const uint32_t* consts, uint32_t n_consts, uint32_t n_vars,
                                   uint32_t tape, const uint32_t* assign, uint64_t rows,
                                   uint32_t n_tables, const uint32_t* counts, const uint32_t* nws,
                                   const uint64_t* key_offsets, const uint32_t* keys,
                                   uint64_t n_key_limbs, const uint64_t* value_offsets,
                                   const uint32_t* values, uint64_t n_value_limbs,
                                   const uint32_t* else_values, uint32_t* out,
                                   uint32_t* features_out, char* err, int errlen) {
    std::vector<uint32_t> packed;
    std::string e;
    if (int32_t r = pack_tables(n_tables, counts, nws, key_offsets, keys, n_key_limbs,
                                value_offsets, values, n_value_limbs, else_values, packed, e)) {
        snprintf(err, errlen, "%s", e.c_str());
        return r;
    }
    if (tape >= n_tapes) {
        snprintf(err, errlen, "tape out of range");
        return MH_E_INVALID;
    }
    // what mh_eval_values_tables checks before a launch: every lookup names a table of the set,
    // with the key's word count
    std::vector<std::pair<uint32_t, uint32_t>> lk;
    tape_lookups(nodes + offs[tape], (size_t)(offs[tape + 1] - offs[tape]), lk);
    for (const auto& x : lk)
        if (x.first >= n_tables || x.second != nws[x.first]) {
            snprintf(err, errlen, "lookup of table %u with %u key words", x.first, x.second);
            return MH_E_INVALID;
        }
    std::vector<uint32_t> dconsts, words;
    mh::ConstIndex dindex;
    CompiledTape ct;
    if (int32_t r = compile_tape(nodes + offs[tape], (size_t)(offs[tape + 1] - offs[tape]), consts,
                                 n_consts, n_vars, dconsts, dindex, words, ct, e)) {
        snprintf(err, errlen, "%s", e.c_str());
        return r;
    }
    if (features_out) *features_out = ct.features;
    const uint32_t n_pre = n_vars <= MH_MAX_PRELOAD ? n_vars : 0;
    const u32 nrx = mh_nrx_of(ct.n_regs);
    for (uint64_t row = 0; row < rows; ++row) {
        TableMachine m;
        memset(m.R, 0xCD, sizeof(m.R));
        m.nrx_ = nrx;
        m.slots = words.data();
        m.assign = assign;
        m.cap = rows;
        m.row = row;
        m.tables = packed.data();
        for (uint32_t v = 0; v < n_pre; ++v)
            for (int k = 0; k < 8; ++k) m.R[v][k] = assign[((u64)v * 8 + k) * rows + row];
        u32 s = 0;
        for (;;) {
            if (s >= ct.n_insns) {
                snprintf(err, errlen, "tape ran past its slots");
                return MH_E_INVALID;
            }
            const u32 w0 = words[2 * s], w1 = words[2 * s + 1];
            const u32 op = w1 & 0xFFu;
            if (op == D_END) break;
            if (op == D_WINDOW) {
                s = (s / MH_WINDOW + 1) * MH_WINDOW;
                continue;
            }
            s += step<F_DIV | F_KECCAK | F_EVM | F_CPLX | F_TABLE, true>(m, w0, w1, s);
            if (op == D_BANDZ && (m.R[nrx][0] & 1u) == 0) break;
        }
        u32 res[8];
        memcpy(res, m.R[nrx], 32);
        if (ct.root_bool) {
            res[0] &= 1u;
            for (int k = 1; k < 8; ++k) res[k] = 0;
        }
        for (int k = 0; k < 8; ++k) out[(u64)k * rows + row] = res[k];
    }
    return MH_OK;
}

#ifdef LOOKUP_EMU_MAIN
// Stand-alone driver: tables of 0..65 entries with 1..3 key words, every key and its neighbours
// looked up through compiled tapes (value and hit forms, range widths 8 / 160 / 256), and every
// refusal of pack_tables.  Prints "lookups=N refusals=M" and exits 0 when every value matches a
// linear search.
namespace {

struct Tab {
    uint32_t nw;
    std::vector<std::vector<uint32_t>> keys;  // ascending
    std::vector<std::vector<uint32_t>> vals;
    uint32_t els[8];
};

uint64_t g_s = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_s ^= g_s << 13;
    g_s ^= g_s >> 7;
    g_s ^= g_s << 17;
    return (uint32_t)(g_s >> 16);
}

bool less_key(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
    for (size_t j = a.size(); j-- > 0;)
        if (a[j] != b[j]) return a[j] < b[j];
    return false;
}

int fail(const char* what, long a = 0, long b = 0) {
    fprintf(stderr, "lookup_emu: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

}  // namespace

int main() {
    long lookups = 0, refusals = 0;
    const uint32_t sizes[] = {0, 1, 2, 3, 64, 65};
    const uint32_t ranges[] = {8, 160, 256};
    for (uint32_t nw = 1; nw <= 3; ++nw)
        for (uint32_t n : sizes)
            for (uint32_t range : ranges) {
                Tab tb;
                tb.nw = nw;
                // keys that differ in limb 0 (within a group of 8) and in the top limb of the top
                // word (between groups): the order is decided by the top limb first
                for (uint32_t i = 0; i < n; ++i) {
                    std::vector<uint32_t> k(8 * nw, 0u);
                    k[0] = 2 * (n - i) + 2;
                    k[8 * nw - 1] = (i / 8) + 1;
                    tb.keys.push_back(k);
                }
                std::sort(tb.keys.begin(), tb.keys.end(), less_key);
                for (uint32_t i = 0; i < n; ++i) {
                    std::vector<uint32_t> v(8, 0u);
                    for (uint32_t j = 0; j < 8; ++j) v[j] = j * 32 < range ? rnd() : 0u;
                    if (range % 32) v[range / 32] &= (1u << (range % 32)) - 1u;
                    tb.vals.push_back(v);
                }
                for (uint32_t j = 0; j < 8; ++j) tb.els[j] = j * 32 < range ? 0xE15E0000u + j : 0u;
                if (range % 32) tb.els[range / 32] &= (1u << (range % 32)) - 1u;
                // probe keys: every entry, one below and one above it, zero and all-ones
                std::vector<std::vector<uint32_t>> probes;
                probes.push_back(std::vector<uint32_t>(8 * nw, 0u));
                probes.push_back(std::vector<uint32_t>(8 * nw, ~0u));
                for (const auto& k : tb.keys) {
                    probes.push_back(k);
                    auto lo = k, hi = k;
                    lo[0] -= 1;
                    hi[0] += 1;
                    probes.push_back(lo);
                    probes.push_back(hi);
                    auto top = k;
                    top[8 * nw - 1] += 1;
                    probes.push_back(top);
                }
                const uint64_t rows = probes.size();
                // tape: key = concat of nw 256-bit columns (column 0 the low word)
                std::vector<mh_node> t;
                for (uint32_t w = 0; w < nw; ++w) {
                    mh_node v{};
                    v.op = MH_OP_VAR;
                    v.width = 256;
                    v.imm0 = w;
                    t.push_back(v);
                }
                uint32_t key = 0;
                for (uint32_t w = 1; w < nw; ++w) {
                    mh_node c{};
                    c.op = MH_OP_CONCAT;
                    c.width = (uint16_t)(256 * (w + 1));
                    c.a = w;  // high part: the next column
                    c.b = key;
                    key = (uint32_t)t.size();
                    t.push_back(c);
                }
                for (int hit = 0; hit < 2; ++hit) {
                    std::vector<mh_node> tp = t;
                    mh_node l{};
                    l.op = MH_OP_LOOKUP;
                    l.width = hit ? 0 : (uint16_t)range;
                    l.a = key;
                    l.imm0 = 0;
                    l.imm1 = (uint32_t)hit;
                    tp.push_back(l);
                    const uint64_t offs[2] = {0, tp.size()};
                    std::vector<uint32_t> assign((size_t)nw * 8 * rows), kk, vv, out(8 * rows);
                    for (uint64_t r = 0; r < rows; ++r)
                        for (uint32_t j = 0; j < 8 * nw; ++j)
                            assign[((size_t)(j / 8) * 8 + j % 8) * rows + r] = probes[r][j];
                    for (const auto& k : tb.keys) kk.insert(kk.end(), k.begin(), k.end());
                    for (const auto& v : tb.vals) vv.insert(vv.end(), v.begin(), v.end());
                    const uint32_t counts[1] = {n}, nws[1] = {nw}, zero_const[8] = {0};
                    const uint64_t ko[1] = {0}, vo[1] = {0};
                    char err[256] = "";
                    uint32_t feats = 0;
                    const int32_t rc = lookup_emu_eval(
                        tp.data(), offs, 1, zero_const, 1, nw, 0, assign.data(), rows, 1, counts,
                        nws, ko, kk.data(), kk.size(), vo, vv.data(), vv.size(), tb.els,
                        out.data(), &feats, err, sizeof err);
                    if (rc != MH_OK) return fail(err, rc, nw);
                    if (!(feats & F_TABLE)) return fail("tape without F_TABLE", feats);
                    for (uint64_t r = 0; r < rows; ++r) {
                        long at = -1;
                        for (uint32_t i = 0; i < n; ++i)
                            if (tb.keys[i] == probes[r]) at = i;
                        for (int k = 0; k < 8; ++k) {
                            const uint32_t want = hit ? (k == 0 && at >= 0)
                                                      : at >= 0 ? tb.vals[at][k] : tb.els[k];
                            if (out[(size_t)k * rows + r] != want) return fail("value", n, (long)r);
                        }
                        ++lookups;
                    }
                }
            }
    // refusals of the validation
    {
        std::vector<uint32_t> out;
        std::string e;
        const uint32_t k2[16] = {5, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0};  // descending
        const uint32_t keq[16] = {5, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0};  // repeated
        const uint32_t v2[16] = {0}, els[8] = {0};
        const uint64_t o0[1] = {0}, o9[1] = {9};
        const uint32_t c2[1] = {2}, n1[1] = {1}, n0[1] = {0}, n4[1] = {4};
        if (pack_tables(1, c2, n1, o0, k2, 16, o0, v2, 16, els, out, e) != MH_E_INVALID) return fail("unsorted");
        ++refusals;
        if (pack_tables(1, c2, n1, o0, keq, 16, o0, v2, 16, els, out, e) != MH_E_INVALID) return fail("repeated");
        ++refusals;
        if (pack_tables(1, c2, n0, o0, keq, 16, o0, v2, 16, els, out, e) != MH_E_INVALID) return fail("nw 0");
        ++refusals;
        if (pack_tables(1, c2, n4, o0, keq, 64, o0, v2, 16, els, out, e) != MH_E_INVALID) return fail("nw 4");
        ++refusals;
        if (pack_tables(1, c2, n1, o9, keq, 16, o0, v2, 16, els, out, e) != MH_E_INVALID) return fail("key offset");
        ++refusals;
        if (pack_tables(1, c2, n1, o0, keq, 16, o9, v2, 16, els, out, e) != MH_E_INVALID) return fail("value offset");
        ++refusals;
        if (pack_tables(1, c2, n1, o0, keq, 15, o0, v2, 16, els, out, e) != MH_E_INVALID) return fail("short keys");
        ++refusals;
        const uint32_t kasc[16] = {3, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0};
        if (pack_tables(1, c2, n1, o0, kasc, 16, o0, v2, 16, els, out, e) != MH_OK) return fail("valid refused");
        if (pack_tables(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, out, e) != MH_OK)
            return fail("empty set refused");
    }
    printf("lookups=%ld refusals=%ld\n", lookups, refusals);
    return 0;
}
#endif
