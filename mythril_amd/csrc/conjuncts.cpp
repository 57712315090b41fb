// Conjunct plan of a query's root tape (mh_conjuncts_build, include/mythril_hip.h): one
// self-contained tape per AND leaf, for the repair step's per-row conjunct scores (repair.hip).
// Host only: no device, no HIP runtime.  The leaves are flattened as harvest.cpp conjuncts(root)
// flattens them (the harvest tags its sets with these node ids) and each leaf's cone is re-indexed
// as compile.cpp split_conjunction re-indexes a part: its nodes in ascending order.
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/mythril_hip.h"

int32_t mh_detail_set_err(int32_t code, const char* msg);  // capi.cpp

struct mh_conjuncts {  // owns the arrays an mh_conjuncts_info points into
    std::vector<mh_node> nodes;
    std::vector<uint64_t> tape_off;
    std::vector<uint32_t> leaf, col_off, cols;
};

namespace {

int arity(uint8_t op) {  // tape.py ARITY (lowered tapes hold no host-only ops)
    switch (op) {
        case MH_OP_CONST: case MH_OP_VAR: case MH_OP_TRUE: case MH_OP_FALSE: return 0;
        case MH_OP_BVNEG: case MH_OP_BVNOT: case MH_OP_NOT: case MH_OP_EXTRACT: case MH_OP_ZEXT:
        case MH_OP_SEXT: case MH_OP_KECCAK: return 1;
        case MH_OP_ITE: case MH_OP_EVM_ADDMOD: case MH_OP_EVM_MULMOD: return 3;
        default: return 2;
    }
}

}  // namespace

extern "C" int32_t mh_conjuncts_build(const mh_node* nodes, uint32_t n_nodes,
                                      const uint32_t* group_cols, uint32_t n_group_cols,
                                      uint32_t max_conjuncts, mh_conjuncts** out,
                                      mh_conjuncts_info* info) {
    if (!out || !info) return mh_detail_set_err(MH_E_INVALID, "null out pointer");
    *out = nullptr;
    if (!nodes || !n_nodes || (n_group_cols && !group_cols))
        return mh_detail_set_err(MH_E_INVALID, "null or empty argument");
    try {
        for (uint32_t i = 0; i < n_nodes; ++i) {
            const mh_node& s = nodes[i];
            const int k = arity(s.op);
            if ((k >= 1 && s.a >= i) || (k >= 2 && s.b >= i) || (k >= 3 && s.c >= i))
                return mh_detail_set_err(MH_E_INVALID, "malformed tape node");
        }
        if (nodes[n_nodes - 1].width != 0)
            return mh_detail_set_err(MH_E_INVALID, "the root is not a Bool");
        std::vector<uint32_t> conj, st{n_nodes - 1};
        while (!st.empty()) {  // harvest.cpp conjuncts(root): the AND leaves, left to right
            const uint32_t n = st.back();
            st.pop_back();
            if (nodes[n].op == MH_OP_AND) {
                st.push_back(nodes[n].b);
                st.push_back(nodes[n].a);
            } else {
                conj.push_back(n);
            }
        }
        std::vector<uint32_t> want(group_cols, group_cols + n_group_cols);
        std::sort(want.begin(), want.end());
        auto r = new mh_conjuncts();
        struct Guard {
            mh_conjuncts* p;
            ~Guard() { delete p; }
        } guard{r};
        r->tape_off.push_back(0);
        r->col_off.push_back(0);
        std::vector<uint32_t> mark(n_nodes, UINT32_MAX), idx(n_nodes, 0), keep, cols;
        for (uint32_t ci = 0; ci < (uint32_t)conj.size(); ++ci) {
            keep.clear();
            cols.clear();
            st.assign(1, conj[ci]);
            while (!st.empty()) {  // the leaf's cone and the columns it reads
                const uint32_t u = st.back();
                st.pop_back();
                if (mark[u] == ci) continue;
                mark[u] = ci;
                keep.push_back(u);
                if (nodes[u].op == MH_OP_VAR) cols.push_back(nodes[u].imm0);
                const int k = arity(nodes[u].op);
                if (k >= 1) st.push_back(nodes[u].a);
                if (k >= 2) st.push_back(nodes[u].b);
                if (k >= 3) st.push_back(nodes[u].c);
            }
            std::sort(cols.begin(), cols.end());
            cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
            bool reads = !cols.empty();
            if (reads && n_group_cols) {
                reads = false;
                for (uint32_t c : cols)
                    if (std::binary_search(want.begin(), want.end(), c)) reads = true;
            }
            if (!reads) continue;
            if (r->leaf.size() >= max_conjuncts)
                return mh_detail_set_err(MH_E_UNSUPPORTED, "more conjuncts than max_conjuncts");
            std::sort(keep.begin(), keep.end());  // the leaf is its cone's last node
            for (uint32_t u : keep) {
                mh_node x = nodes[u];
                const int k = arity(x.op);
                if (k >= 1) x.a = idx[x.a];
                if (k >= 2) x.b = idx[x.b];
                if (k >= 3) x.c = idx[x.c];
                idx[u] = (uint32_t)(r->nodes.size() - r->tape_off.back());
                r->nodes.push_back(x);
            }
            r->tape_off.push_back(r->nodes.size());
            r->leaf.push_back(conj[ci]);
            r->cols.insert(r->cols.end(), cols.begin(), cols.end());
            r->col_off.push_back((uint32_t)r->cols.size());
        }
        if (r->leaf.size() < 2)
            return mh_detail_set_err(MH_E_UNSUPPORTED, "fewer than two conjuncts read the columns");
        if (r->cols.empty()) r->cols.push_back(0);
        info->nodes = r->nodes.data();
        info->tape_off = r->tape_off.data();
        info->leaf = r->leaf.data();
        info->col_off = r->col_off.data();
        info->cols = r->cols.data();
        info->n_conjuncts = (uint32_t)r->leaf.size();
        info->pad = 0;
        guard.p = nullptr;
        *out = r;
        return MH_OK;
    } catch (const std::bad_alloc&) {
        return mh_detail_set_err(MH_E_NOMEM, "host allocation failed");
    }
}

extern "C" int32_t mh_conjuncts_free(mh_conjuncts* c) {
    delete c;
    return MH_OK;
}
