// Reading a Bool tape node as a bound of one term against a constant: t == c, the unsigned
// comparisons either way round, and smt.py's ULE / UGE (bitvec_helper.py: Or(ULT(a, b), a == b)).
// Shared by refuted() (query.cpp), which pins any term to a range, and the domain analysis
// (domains.cpp), which keeps the bounds of plain VAR nodes.  Host only.
#pragma once
#include <stdint.h>

#include <utility>

#include "../../include/mythril_hip.h"

namespace mh {
namespace bound {

struct Cmp {
    uint8_t op;     // MH_OP_EQ or MH_OP_BVULT .. MH_OP_BVUGE, read as t op c
    uint32_t t, c;  // tape nodes: the term, the constant
};

// t op c for a comparison node of a bit-vector term t with a constant c (either side; a constant on
// the left mirrors the comparison)
inline bool cmp_of_plain(const mh_node* tape, uint32_t n, Cmp& out) {
    const mh_node& x = tape[n];
    uint8_t op = x.op;
    if (op != MH_OP_EQ && !(op >= MH_OP_BVULT && op <= MH_OP_BVUGE)) return false;
    const bool ca = tape[x.a].op == MH_OP_CONST, cb = tape[x.b].op == MH_OP_CONST;
    if (ca == cb || tape[x.a].width == 0) return false;
    if (ca)
        op = op == MH_OP_BVULT ? MH_OP_BVUGT : op == MH_OP_BVULE ? MH_OP_BVUGE
           : op == MH_OP_BVUGT ? MH_OP_BVULT : op == MH_OP_BVUGE ? MH_OP_BVULE : op;
    out = {op, ca ? x.b : x.a, ca ? x.a : x.b};
    return true;
}

// the same, with Or(ULT(t, c), t == c) read as BVULE and Or(UGT(t, c), t == c) as BVUGE
inline bool cmp_of(const mh_node* tape, uint32_t n, Cmp& out) {
    const mh_node& x = tape[n];
    if (x.op == MH_OP_OR) {
        Cmp p, e;
        if (!cmp_of_plain(tape, x.a, p) || !cmp_of_plain(tape, x.b, e)) return false;
        if (p.op == MH_OP_EQ) std::swap(p, e);
        if (e.op != MH_OP_EQ || p.t != e.t || p.c != e.c) return false;
        if (p.op != MH_OP_BVULT && p.op != MH_OP_BVUGT) return false;
        out = {(uint8_t)(p.op == MH_OP_BVULT ? MH_OP_BVULE : MH_OP_BVUGE), p.t, p.c};
        return true;
    }
    return cmp_of_plain(tape, n, out);
}

// the comparison a negated one states: not (t < c) is t >= c, ...; EQ stays (the caller reads a
// negated equality as a disequality)
inline uint8_t negated(uint8_t op) {
    return op == MH_OP_BVULT ? MH_OP_BVUGE : op == MH_OP_BVULE ? MH_OP_BVUGT
         : op == MH_OP_BVUGT ? MH_OP_BVULE : op == MH_OP_BVUGE ? MH_OP_BVULT : op;
}

}  // namespace bound
}  // namespace mh
