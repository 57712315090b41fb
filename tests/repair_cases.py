"""Queries for the repair step's tests (test infrastructure only).

``chain_query(M)``: M 256-bit symbols with ``(x_i ^ A_i) == K_i`` (random 256-bit constants)
chained by ``Not(x_i == x_{i+1})`` -- one column-connected group of 2M - 1 conjuncts whose
harvested sets override each other: every conjunct's set is in the guide with probability
208/256, and the disequalities' sets overwrite the equalities' columns, so a 256-row round misses
(DESIGN §6 "repair", §10.7).
"""
import random

from mythril_amd import smt
from mythril_amd.smt import Not, symbol_factory


def chain_query(m: int, seed: int = 0xC4A1):
    """(term context, constraints) of the M-symbol chain."""
    rng = random.Random(seed * 1000 + m)
    ctx = smt.set_context(smt.Context())
    xs = [symbol_factory.BitVecSym("x%d" % i, 256) for i in range(m)]
    cs = []
    for x in xs:
        a = symbol_factory.BitVecVal(rng.getrandbits(256), 256)
        k = symbol_factory.BitVecVal(rng.getrandbits(256), 256)
        cs.append((x ^ a) == k)
    for p, q in zip(xs, xs[1:]):
        cs.append(Not(p == q))
    return ctx, cs
