// Replays recorded root tapes against the host-only side of the repair step -- the conjunct plan
// (csrc/conjuncts.cpp mh_conjuncts_build) and the guide harvest with its set provenance
// (csrc/harvest.cpp mh_guide_harvest + mh_harvest_set_conjuncts) -- and reads every returned
// array end to end.  Built with -fsanitize=address,undefined by tests/test_repair_host.py.
//
// File: u32 words, little-endian.  n_records, then per record: n_nodes, n_consts, n_cols,
// n_group_cols, the nodes (6 words each), the constants (8 words each), the column widths and the
// group's columns (one word each).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mythril_hip.h"

static std::string g_err;
int32_t mh_detail_set_err(int32_t code, const char* msg) {  // capi.cpp's, for this build
    g_err = msg;
    return code;
}

static uint64_t g_sum = 0;  // every word read goes in: nothing is optimised away

static int fail(const char* what, uint32_t rec) {
    std::fprintf(stderr, "record %u: %s (%s)\n", rec, what, g_err.c_str());
    return 1;
}

// the plan's arrays read end to end; the structure checked
static int read_plan(const mh_conjuncts_info& info, uint32_t n_nodes, uint32_t n_cols, uint32_t rec) {
    if (info.n_conjuncts < 2 || info.tape_off[0] != 0 || info.col_off[0] != 0)
        return fail("plan header", rec);
    for (uint32_t i = 0; i < info.n_conjuncts; ++i) {
        const uint64_t b = info.tape_off[i], e = info.tape_off[i + 1];
        if (e <= b || info.leaf[i] >= n_nodes) return fail("plan tape range", rec);
        for (uint64_t k = b; k < e; ++k) {
            const mh_node& x = info.nodes[k];
            g_sum += x.op + x.width + x.a + x.b + x.c + x.imm0 + x.imm1;
        }
        if (info.nodes[e - 1].width != 0) return fail("plan tape root is not a Bool", rec);
        if (info.col_off[i + 1] <= info.col_off[i]) return fail("conjunct without columns", rec);
        for (uint32_t q = info.col_off[i]; q < info.col_off[i + 1]; ++q) {
            if (info.cols[q] >= n_cols) return fail("plan column out of range", rec);
            if (q > info.col_off[i] && info.cols[q] <= info.cols[q - 1])
                return fail("plan columns not ascending", rec);
            g_sum += info.cols[q];
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint32_t> w;
    uint32_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
    std::fclose(f);
    size_t p = 0;
    const uint32_t n_rec = w.at(p++);
    uint32_t plans = 0, refused = 0, guides = 0, tagged = 0;
    for (uint32_t rec = 0; rec < n_rec; ++rec) {
        const uint32_t n_nodes = w.at(p), n_consts = w.at(p + 1), n_cols = w.at(p + 2),
                       n_gc = w.at(p + 3);
        p += 4;
        std::vector<mh_node> nodes(n_nodes);
        std::memcpy(nodes.data(), &w.at(p), (size_t)n_nodes * sizeof(mh_node));
        p += (size_t)n_nodes * 6;
        std::vector<uint32_t> consts(w.begin() + (long)p, w.begin() + (long)(p + 8ull * n_consts));
        p += 8ull * n_consts;
        std::vector<uint16_t> widths(n_cols);
        for (uint32_t c = 0; c < n_cols; ++c) widths[c] = (uint16_t)w.at(p + c);
        p += n_cols;
        std::vector<uint32_t> gc(w.begin() + (long)p, w.begin() + (long)(p + n_gc));
        p += n_gc;

        // the plan: every kept leaf, the group's, and both refusals
        for (int pass = 0; pass < 2; ++pass) {
            mh_conjuncts* h = nullptr;
            mh_conjuncts_info info{};
            const int32_t r = mh_conjuncts_build(nodes.data(), n_nodes, pass ? gc.data() : nullptr,
                                                 pass ? n_gc : 0, 4096, &h, &info);
            if (r == MH_OK) {
                if (read_plan(info, n_nodes, n_cols, rec)) return 1;
                ++plans;
                const uint32_t nc = info.n_conjuncts;
                mh_conjuncts_free(h);
                mh_conjuncts* h2 = nullptr;  // one fewer than it needs: refused, nothing returned
                if (mh_conjuncts_build(nodes.data(), n_nodes, pass ? gc.data() : nullptr,
                                       pass ? n_gc : 0, nc - 1, &h2, &info) != MH_E_UNSUPPORTED || h2)
                    return fail("max_conjuncts not enforced", rec);
                ++refused;
            } else if (r == MH_E_UNSUPPORTED) {
                if (h) return fail("a refused plan returned a handle", rec);
                ++refused;
            } else {
                return fail("mh_conjuncts_build", rec);
            }
        }
        const uint32_t none_col = n_cols;  // a column no leaf reads: fewer than two leaves kept
        mh_conjuncts* h3 = nullptr;
        mh_conjuncts_info i3{};
        if (mh_conjuncts_build(nodes.data(), n_nodes, &none_col, 1, 4096, &h3, &i3) !=
            MH_E_UNSUPPORTED)
            return fail("a group no leaf reads was not refused", rec);

        // the harvest and its tags
        mh_harvest* hv = nullptr;
        mh_guide g{};
        if (mh_guide_harvest(nodes.data(), n_nodes, consts.data(), n_consts, widths.data(), n_cols,
                             nullptr, nullptr, 0, &hv, &g) != MH_OK)
            return fail("mh_guide_harvest", rec);
        ++guides;
        std::vector<uint32_t> tags(g.n_sets + 1, 0);
        if (mh_harvest_set_conjuncts(hv, tags.data(), g.n_sets) != MH_OK)
            return fail("mh_harvest_set_conjuncts", rec);
        if (mh_harvest_set_conjuncts(hv, tags.data(), g.n_sets + 1) != MH_E_INVALID)
            return fail("a wrong n_sets was not refused", rec);
        for (uint32_t j = 0; j < g.n_sets; ++j) {
            if (tags[j] != MH_NO_CONJUNCT) {
                if (tags[j] >= n_nodes) return fail("tag out of range", rec);
                ++tagged;
            }
            for (uint32_t a = g.set_off[j]; a < g.set_off[j + 1]; ++a)
                for (uint32_t e = g.alt_off[a]; e < g.alt_off[a + 1]; ++e) {
                    g_sum += g.entry_col[e];
                    for (int k = 0; k < 8; ++k) g_sum += g.entry_val[8ull * e + k];
                }
            g_sum += g.set_prob[j];
        }
        mh_harvest_free(hv);
    }
    std::printf("records=%u plans=%u refused=%u guides=%u tagged=%u sum=%llu\n", n_rec, plans,
                refused, guides, tagged, (unsigned long long)(g_sum & 0xFFFF));
    return 0;
}
