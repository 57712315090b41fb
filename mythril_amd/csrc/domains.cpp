// Finite domains of a group's columns (mh_domains_*; DESIGN.md §6 "Decision by enumeration").
//
// mh_domains_build reads, per column of one group, a superset of the values the column takes in any
// row that satisfies the group's tape, from the top-level conjuncts over the plain VAR node alone:
// the column width, v == c, an OR tree of v == c_k, unsigned bounds against constants (the reading
// refuted() does, bound_read.h) and v != c.  Everything is intersected; a conjunct of any other
// shape contributes nothing, so the result can only be too large, never too small.  The cross
// product of the domains is what the enumerating generator writes (enumerate.hip).
// mh_domains_create builds the same handle from plain arrays, validated.  Host only: no device
// is touched here (the generator parks its device copy in the handle, domains.h).
#include "domains.h"

#include <algorithm>
#include <cstring>
#include <iterator>
#include <new>
#include <string>

#include "bound_read.h"

int32_t mh_detail_set_err(int32_t code, const char* msg);  // capi.cpp

namespace {

struct V {  // a 256-bit value, little-endian u32 limbs
    uint32_t w[8] = {};
    bool operator==(const V& o) const { return std::memcmp(w, o.w, sizeof w) == 0; }
    bool operator<(const V& o) const {
        for (int i = 7; i >= 0; --i)
            if (w[i] != o.w[i]) return w[i] < o.w[i];
        return false;
    }
    bool zero() const {
        for (uint32_t x : w)
            if (x) return false;
        return true;
    }
};

V load(const uint32_t* p) {
    V v;
    std::memcpy(v.w, p, sizeof v.w);
    return v;
}

V ones(uint32_t bits) {  // 2^bits - 1, bits <= 256
    V r;
    for (uint32_t i = 0; i < bits / 32; ++i) r.w[i] = ~0u;
    if (bits % 32) r.w[bits / 32] = (1u << (bits % 32)) - 1u;
    return r;
}

// a + x; *carry = the sum left 256 bits
V plus(const V& a, uint64_t x, bool* carry) {
    V r;
    uint64_t c = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t add = i == 0 ? (uint32_t)x : i == 1 ? (uint32_t)(x >> 32) : 0u;
        const uint64_t s = (uint64_t)a.w[i] + add + c;
        r.w[i] = (uint32_t)s;
        c = s >> 32;
    }
    *carry = c != 0;
    return r;
}

V minus_one(const V& a) {  // a != 0
    V r = a;
    for (int i = 0; i < 8; ++i)
        if (r.w[i]-- != 0) break;
    return r;
}

// hi - lo + 1 for lo <= hi, saturating at 2^64 - 1
uint64_t span(const V& lo, const V& hi) {
    uint32_t d[8];
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t s = (uint64_t)hi.w[i] - lo.w[i] - borrow;
        d[i] = (uint32_t)s;
        borrow = (s >> 32) & 1u;
    }
    for (int i = 2; i < 8; ++i)
        if (d[i]) return UINT64_MAX;
    const uint64_t d64 = (uint64_t)d[1] << 32 | d[0];
    return d64 == UINT64_MAX ? UINT64_MAX : d64 + 1;
}

uint64_t mul_sat(uint64_t a, uint64_t b) {
    if (a == 0 || b == 0) return 0;
    return a > UINT64_MAX / b ? UINT64_MAX : a * b;
}

int32_t fail(const std::string& m) { return mh_detail_set_err(MH_E_INVALID, m.c_str()); }

struct ColState {
    V lo, hi;
    bool empty = false, has_list = false;
    std::vector<V> list;  // ascending, distinct
    std::vector<V> ne;    // values the column must differ from
};

void push_column(mh_domains& d, uint32_t col, uint32_t kind, uint64_t size, const V& lo,
                 const std::vector<V>& list) {
    d.cols.push_back(col);
    d.kind.push_back(kind);
    d.size.push_back(size);
    d.lo.insert(d.lo.end(), lo.w, lo.w + 8);
    for (const V& v : list) d.list_vals.insert(d.list_vals.end(), v.w, v.w + 8);
    d.list_off.push_back((uint32_t)(d.list_vals.size() / 8));
}

void finish(mh_domains& d) {
    bool any_empty = false;
    uint64_t rows = 1;
    for (uint64_t s : d.size) {
        any_empty |= s == 0;
        rows = mul_sat(rows, std::max<uint64_t>(s, 1));
    }
    d.rows = any_empty ? 0 : rows;
}

}  // namespace

extern "C" {

int32_t mh_domains_build(const mh_node* nodes, uint32_t n_nodes, const uint32_t* consts,
                         uint32_t n_consts, const uint16_t* col_width, uint32_t n_widths,
                         const uint32_t* group_cols, uint32_t n_group_cols, mh_domains** out) {
    if (!out) return fail("mh_domains_build: null out");
    *out = nullptr;
    if (!nodes || n_nodes == 0 || !col_width || (n_consts && !consts) ||
        (n_group_cols && !group_cols))
        return fail("mh_domains_build: null argument");
    if (nodes[n_nodes - 1].width != 0) return fail("mh_domains_build: the root is not Bool");
    // every node the reading below follows an operand of, or takes a column / constant from
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const mh_node& x = nodes[i];
        const bool binary = x.op == MH_OP_AND || x.op == MH_OP_OR || x.op == MH_OP_EQ ||
                            (x.op >= MH_OP_BVULT && x.op <= MH_OP_BVUGE);
        if ((binary || x.op == MH_OP_NOT) && (x.a >= i || (binary && x.b >= i)))
            return fail("mh_domains_build: operand of node " + std::to_string(i) +
                        " is not an earlier node");
        if (x.op == MH_OP_VAR && x.imm0 >= n_widths)
            return fail("mh_domains_build: node " + std::to_string(i) +
                        " reads a column outside the widths");
        if (x.op == MH_OP_CONST && x.imm0 >= n_consts)
            return fail("mh_domains_build: node " + std::to_string(i) +
                        " reads a constant outside the pool");
    }
    // the group's columns, ascending (none: a ground group, whose product is the one empty row)
    std::vector<uint32_t> cols(group_cols, group_cols + n_group_cols);
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    std::vector<int32_t> slot(n_widths, -1);
    std::vector<ColState> st(cols.size());
    for (size_t j = 0; j < cols.size(); ++j) {
        const uint32_t c = cols[j];
        if (c >= n_widths) return fail("mh_domains_build: group column outside the widths");
        if (col_width[c] == 0 || col_width[c] > 256)
            return fail("mh_domains_build: column width outside 1..256");
        slot[c] = (int32_t)j;
        st[j].hi = ones(col_width[c]);
    }
    // the state of the column a plain VAR node names, when it is one of the group's
    auto state_of = [&](uint32_t t) -> ColState* {
        const mh_node& v = nodes[t];
        if (v.op != MH_OP_VAR || slot[v.imm0] < 0 || v.width != col_width[v.imm0]) return nullptr;
        return &st[slot[v.imm0]];
    };
    // the AND leaves, left to right (as the guide harvest flattens them)
    std::vector<uint32_t> stack{n_nodes - 1}, leaves;
    while (!stack.empty()) {
        const uint32_t x = stack.back();
        stack.pop_back();
        if (nodes[x].op == MH_OP_AND) {
            stack.push_back(nodes[x].b);
            stack.push_back(nodes[x].a);
        } else {
            leaves.push_back(x);
        }
    }
    using mh::bound::Cmp;
    std::vector<V> alts;
    for (uint32_t leaf : leaves) {
        bool neg = false;
        uint32_t n = leaf;
        if (nodes[n].op == MH_OP_NOT) {
            neg = true;
            n = nodes[n].a;
        }
        Cmp k;
        if (mh::bound::cmp_of(nodes, n, k)) {
            ColState* s = state_of(k.t);
            if (!s) continue;
            const V c = load(consts + 8 * (size_t)nodes[k.c].imm0);
            const uint8_t op = neg ? mh::bound::negated(k.op) : k.op;
            if (op == MH_OP_EQ && neg) {
                s->ne.push_back(c);
                continue;
            }
            if (op == MH_OP_EQ || op == MH_OP_BVULE || op == MH_OP_BVULT) {  // an upper bound
                if (op == MH_OP_BVULT && c.zero()) {
                    s->empty = true;
                    continue;
                }
                const V h = op == MH_OP_BVULT ? minus_one(c) : c;
                if (h < s->hi) s->hi = h;
            }
            if (op == MH_OP_EQ || op == MH_OP_BVUGE || op == MH_OP_BVUGT) {  // a lower bound
                V l = c;
                if (op == MH_OP_BVUGT) {
                    bool carry;
                    l = plus(c, 1, &carry);
                    if (carry) {
                        s->empty = true;
                        continue;
                    }
                }
                if (s->lo < l) s->lo = l;
            }
            continue;
        }
        if (neg || nodes[n].op != MH_OP_OR) continue;
        // an OR tree whose every leaf is v == c_k for one column v
        ColState* s = nullptr;
        bool ok = true;
        alts.clear();
        stack.assign(1, n);
        while (ok && !stack.empty()) {
            const uint32_t x = stack.back();
            stack.pop_back();
            if (nodes[x].op == MH_OP_OR) {
                stack.push_back(nodes[x].b);
                stack.push_back(nodes[x].a);
                continue;
            }
            Cmp e;
            ColState* sx = nullptr;
            ok = mh::bound::cmp_of_plain(nodes, x, e) && e.op == MH_OP_EQ &&
                 (sx = state_of(e.t)) != nullptr && (s == nullptr || s == sx);
            if (ok) {
                s = sx;
                alts.push_back(load(consts + 8 * (size_t)nodes[e.c].imm0));
            }
        }
        if (!ok || !s) continue;
        std::sort(alts.begin(), alts.end());
        alts.erase(std::unique(alts.begin(), alts.end()), alts.end());
        if (s->has_list) {
            std::vector<V> both;
            std::set_intersection(s->list.begin(), s->list.end(), alts.begin(), alts.end(),
                                  std::back_inserter(both));
            s->list.swap(both);
        } else {
            s->has_list = true;
            s->list = alts;
        }
    }
    mh_domains* d = new (std::nothrow) mh_domains();
    if (!d) return mh_detail_set_err(MH_E_NOMEM, "mh_domains_build: allocation");
    d->list_off.push_back(0);
    for (size_t j = 0; j < cols.size(); ++j) {
        ColState& s = st[j];
        if (s.hi < s.lo) s.empty = true;
        auto excluded = [&](const V& v) {
            return std::find(s.ne.begin(), s.ne.end(), v) != s.ne.end();
        };
        if (s.has_list) {
            std::vector<V> keep;
            for (const V& v : s.list)
                if (!s.empty && !(v < s.lo) && !(s.hi < v) && !excluded(v)) keep.push_back(v);
            push_column(*d, cols[j], MH_DOMAIN_LIST, keep.size(), V(), keep);
            continue;
        }
        // a disequality at an end of the interval trims it (one inside it is ignored)
        while (!s.empty && (excluded(s.lo) || excluded(s.hi))) {
            if (s.lo == s.hi) {
                s.empty = true;
            } else if (excluded(s.lo)) {
                bool carry;
                s.lo = plus(s.lo, 1, &carry);
            } else {
                s.hi = minus_one(s.hi);
            }
        }
        push_column(*d, cols[j], MH_DOMAIN_INTERVAL, s.empty ? 0 : span(s.lo, s.hi),
                    s.empty ? V() : s.lo, {});
    }
    finish(*d);
    *out = d;
    return MH_OK;
}

int32_t mh_domains_create(const uint32_t* cols, const uint32_t* kind, const uint64_t* size,
                          const uint32_t* lo, const uint32_t* list_off, const uint32_t* list_vals,
                          uint32_t n_cols, const uint16_t* col_width, uint32_t n_widths,
                          mh_domains** out) {
    if (!out) return fail("mh_domains_create: null out");
    *out = nullptr;
    if (n_cols == 0) return fail("mh_domains_create: no column");
    if (!cols || !kind || !size || !lo || !list_off || !col_width)
        return fail("mh_domains_create: null argument");
    if (list_off[0] != 0) return fail("mh_domains_create: list_off does not start at 0");
    for (uint32_t j = 0; j < n_cols; ++j) {
        const std::string at = "mh_domains_create: column " + std::to_string(j);
        if (cols[j] >= n_widths) return fail(at + " is outside the widths");
        if (j && cols[j] <= cols[j - 1]) return fail(at + ": columns are not ascending");
        const uint32_t w = col_width[cols[j]];
        if (w == 0 || w > 256) return fail(at + ": width outside 1..256");
        if (list_off[j + 1] < list_off[j]) return fail(at + ": list_off decreases");
        const uint32_t n = list_off[j + 1] - list_off[j];
        const V top = ones(w);
        if (kind[j] == MH_DOMAIN_LIST) {
            if (size[j] != n) return fail(at + ": size is not the list's length");
            if (n && !list_vals) return fail("mh_domains_create: null list_vals");
            for (uint32_t i = 0; i < n; ++i) {
                const V v = load(list_vals + 8 * (size_t)(list_off[j] + i));
                if (top < v) return fail(at + ": a list value exceeds the column's width");
                if (i && !(load(list_vals + 8 * (size_t)(list_off[j] + i - 1)) < v))
                    return fail(at + ": list values are not ascending");
            }
        } else if (kind[j] == MH_DOMAIN_INTERVAL) {
            if (n) return fail(at + ": an interval with list values");
            const V l = load(lo + 8 * (size_t)j);
            if (top < l) return fail(at + ": lo exceeds the column's width");
            if (size[j]) {
                bool carry;
                const V h = plus(l, size[j] - 1, &carry);
                if (carry || top < h) return fail(at + ": lo + size - 1 exceeds the column's width");
            }
        } else {
            return fail(at + ": unknown kind");
        }
    }
    mh_domains* d = new (std::nothrow) mh_domains();
    if (!d) return mh_detail_set_err(MH_E_NOMEM, "mh_domains_create: allocation");
    d->cols.assign(cols, cols + n_cols);
    d->kind.assign(kind, kind + n_cols);
    d->size.assign(size, size + n_cols);
    d->lo.assign(lo, lo + 8 * (size_t)n_cols);
    for (uint32_t j = 0; j < n_cols; ++j)
        if (kind[j] == MH_DOMAIN_LIST) std::fill_n(d->lo.begin() + 8 * (size_t)j, 8, 0u);
    d->list_off.assign(list_off, list_off + n_cols + 1);
    if (list_off[n_cols]) d->list_vals.assign(list_vals, list_vals + 8 * (size_t)list_off[n_cols]);
    finish(*d);
    *out = d;
    return MH_OK;
}

int32_t mh_domains_info(const mh_domains* d, mh_domains_desc* info) {
    if (!d || !info) return fail("mh_domains_info: null argument");
    info->cols = d->cols.data();
    info->kind = d->kind.data();
    info->size = d->size.data();
    info->lo = d->lo.data();
    info->list_off = d->list_off.data();
    info->list_vals = d->list_vals.data();
    info->n_cols = (uint32_t)d->cols.size();
    info->pad = 0;
    info->rows = d->rows;
    return MH_OK;
}

int32_t mh_domains_free(mh_domains* d) {
    if (!d) return MH_OK;
    if (d->dev_release) d->dev_release(d);
    delete d;
    return MH_OK;
}

}  // extern "C"
