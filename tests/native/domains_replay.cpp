// Stand-alone run of the domain analysis (mythril_amd/csrc/domains.cpp) over hand-built tapes of
// the shape cases, for a build with -fsanitize=address,undefined (tests/test_domains.py).  No
// device, no Python: the file has its own main and links domains.cpp alone.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mythril_hip.h"

static std::string g_err;
int32_t mh_detail_set_err(int32_t code, const char* msg) {  // capi.cpp's, for a host-only link
    g_err = msg;
    return code;
}

namespace {

struct Tape {
    std::vector<mh_node> nodes;
    std::vector<uint32_t> consts;  // 8 limbs each
    uint32_t node(uint8_t op, uint16_t width, uint32_t a = 0, uint32_t b = 0, uint32_t imm0 = 0) {
        mh_node n{};
        n.op = op;
        n.width = width;
        n.a = a;
        n.b = b;
        n.imm0 = imm0;
        nodes.push_back(n);
        return (uint32_t)nodes.size() - 1;
    }
    uint32_t var(uint32_t col, uint16_t w) { return node(MH_OP_VAR, w, 0, 0, col); }
    // a constant with every limb `fill` but the lowest, which is `low`
    uint32_t konst(uint16_t w, uint32_t low, uint32_t fill = 0) {
        consts.push_back(low);
        for (int i = 1; i < 8; ++i) consts.push_back(fill);
        return node(MH_OP_CONST, w, 0, 0, (uint32_t)consts.size() / 8 - 1);
    }
    uint32_t cmp(uint8_t op, uint32_t a, uint32_t b) { return node(op, 0, a, b); }
    uint32_t lnot(uint32_t a) { return node(MH_OP_NOT, 0, a); }
};

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL %s (%s)\n", what, g_err.c_str());
        ++failures;
    }
}

// the domains of `t` over `widths`, checked against (kind, size, lo limb 0, list length) of
// column 0 and the row count
void check(const char* what, Tape& t, const std::vector<uint16_t>& widths, uint32_t kind,
           uint64_t size, uint32_t lo0, uint32_t n_list, uint64_t rows) {
    mh_domains* d = nullptr;
    std::vector<uint32_t> cols;
    for (uint32_t c = 0; c < widths.size(); ++c) cols.push_back(c);
    const int32_t r = mh_domains_build(t.nodes.data(), (uint32_t)t.nodes.size(), t.consts.data(),
                                       (uint32_t)t.consts.size() / 8, widths.data(),
                                       (uint32_t)widths.size(), cols.data(),
                                       (uint32_t)cols.size(), &d);
    expect(r == MH_OK && d, what);
    if (r != MH_OK) return;
    mh_domains_desc info;
    expect(mh_domains_info(d, &info) == MH_OK, what);
    expect(info.n_cols == widths.size() && info.kind[0] == kind && info.size[0] == size &&
               info.lo[0] == lo0 && info.list_off[1] - info.list_off[0] == n_list &&
               info.rows == rows,
           what);
    // the same arrays pass the constructor's validation (saturated intervals of narrower
    // columns aside: the constructor takes a size literally)
    if (size != UINT64_MAX) {
        mh_domains* c = nullptr;
        expect(mh_domains_create(info.cols, info.kind, info.size, info.lo, info.list_off,
                                 info.list_vals, info.n_cols, widths.data(),
                                 (uint32_t)widths.size(), &c) == MH_OK,
               what);
        mh_domains_free(c);
    }
    mh_domains_free(d);
}

}  // namespace

int main() {
    const std::vector<uint16_t> w8{8}, w256{256};
    {  // pin
        Tape t;
        t.cmp(MH_OP_EQ, t.var(0, 8), t.konst(8, 5));
        check("pin", t, w8, MH_DOMAIN_INTERVAL, 1, 5, 0, 1);
    }
    {  // Or of three equalities with a duplicate, mirrored operands
        Tape t;
        const uint32_t x = t.var(0, 8);
        const uint32_t a = t.cmp(MH_OP_EQ, x, t.konst(8, 9)), b = t.cmp(MH_OP_EQ, t.konst(8, 2), x),
                       c = t.cmp(MH_OP_EQ, x, t.konst(8, 9));
        t.node(MH_OP_OR, 0, t.node(MH_OP_OR, 0, a, b), c);
        check("or list", t, w8, MH_DOMAIN_LIST, 2, 0, 2, 2);
    }
    {  // bounds both ways round, a negated bound, the Or form of ULE, a disequality at an end
        Tape t;
        const uint32_t x = t.var(0, 8);
        const uint32_t lo = t.cmp(MH_OP_BVULT, t.konst(8, 3), x);            // 3 < x
        const uint32_t hi = t.lnot(t.cmp(MH_OP_BVUGT, x, t.konst(8, 200)));  // not (x > 200)
        const uint32_t k = t.konst(8, 100);
        const uint32_t ule = t.node(MH_OP_OR, 0, t.cmp(MH_OP_BVULT, x, k), t.cmp(MH_OP_EQ, x, k));
        const uint32_t ne = t.lnot(t.cmp(MH_OP_EQ, x, t.konst(8, 4)));
        t.node(MH_OP_AND, 0, t.node(MH_OP_AND, 0, lo, hi), t.node(MH_OP_AND, 0, ule, ne));
        check("bounds", t, w8, MH_DOMAIN_INTERVAL, 96, 5, 0, 96);
    }
    {  // contradicting pins
        Tape t;
        const uint32_t x = t.var(0, 8);
        t.node(MH_OP_AND, 0, t.cmp(MH_OP_EQ, x, t.konst(8, 1)), t.cmp(MH_OP_EQ, x, t.konst(8, 2)));
        check("empty", t, w8, MH_DOMAIN_INTERVAL, 0, 0, 0, 0);
    }
    {  // constants at 2^256 - 1: x > 2^256 - 1 is empty, x >= 2^256 - 3 has three values
        Tape t;
        t.cmp(MH_OP_BVUGT, t.var(0, 256), t.konst(256, ~0u, ~0u));
        check("above the top", t, w256, MH_DOMAIN_INTERVAL, 0, 0, 0, 0);
        Tape u;
        u.cmp(MH_OP_BVUGE, u.var(0, 256), u.konst(256, ~0u - 2, ~0u));
        check("near the top", u, w256, MH_DOMAIN_INTERVAL, 3, ~0u - 2, 0, 3);
    }
    {  // an untouched 256-bit column beside a list: sizes and rows saturate
        Tape t;
        const uint32_t x = t.var(0, 256), y = t.var(1, 8);
        const uint32_t l = t.node(MH_OP_OR, 0, t.cmp(MH_OP_EQ, y, t.konst(8, 1)),
                                  t.cmp(MH_OP_EQ, y, t.konst(8, 2)));
        const uint32_t other = t.cmp(MH_OP_BVSLT, x, t.konst(256, 7));
        t.node(MH_OP_AND, 0, l, other);
        check("saturated", t, {256, 8}, MH_DOMAIN_INTERVAL, UINT64_MAX, 0, 0, UINT64_MAX);
    }
    {  // refusals: a root that is not Bool, a column outside the widths, a forward operand
        Tape t;
        t.var(0, 8);
        mh_domains* d = nullptr;
        expect(mh_domains_build(t.nodes.data(), 1, nullptr, 0, w8.data(), 1, nullptr, 0, &d) ==
                   MH_E_INVALID, "root not Bool");
        Tape u;
        u.cmp(MH_OP_EQ, u.var(3, 8), u.konst(8, 1));
        expect(mh_domains_build(u.nodes.data(), 3, u.consts.data(), 1, w8.data(), 1, nullptr, 0,
                                &d) == MH_E_INVALID, "column outside the widths");
        u.nodes[0].imm0 = 0;
        u.nodes[2].b = 7;
        expect(mh_domains_build(u.nodes.data(), 3, u.consts.data(), 1, w8.data(), 1, nullptr, 0,
                                &d) == MH_E_INVALID, "forward operand");
        expect(mh_domains_build(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, &d) ==
                   MH_E_INVALID, "null tape");
        expect(mh_domains_free(nullptr) == MH_OK, "free(null)");
    }
    if (failures) return 1;
    std::printf("domains_replay ok\n");
    return 0;
}
