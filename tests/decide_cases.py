"""Queries for the decision-by-enumeration tests (test helpers): the random 4-bit family with
its brute-force truth, and hand-built 256-bit queries over tests/laser_like.py's helpers."""
from __future__ import annotations

import itertools
import random

from mythril_amd import smt
from mythril_amd.smt import And, Not, Or, UGE, UGT, ULE, ULT, symbol_factory
from oracle import smt_eval as E
from tests.laser_like import ATTACKER, CREATOR, SOMEGUY, sender_is_actor

NAMES = "xyz"
SEED, COUNT = 20261, 200  # the family the domain and the verdict tests share (truth())


def random_conjunction(rng: random.Random):
    """(context, constraints): 2..6 conjuncts over three 4-bit symbols, the shapes of
    tests/test_query_native.py's refutation family -- equalities, bounds either way round, the
    Or forms of ULE / UGE, negations -- plus disjunctions of equalities and arithmetic conjuncts
    the domain analysis must leave alone."""
    ctx = smt.set_context(smt.Context())
    xs = [symbol_factory.BitVecSym(n, 4) for n in NAMES]

    def const():
        return symbol_factory.BitVecVal(rng.randrange(16), 4)

    def term():
        return rng.choice(xs) if rng.random() < 0.8 else const()

    def atom():
        a, b = term(), term()
        v = rng.choice(xs)
        k = rng.randrange(11)
        c = [lambda: a == b, lambda: ULT(a, b), lambda: UGT(a, b), lambda: ULE(a, b),
             lambda: UGE(a, b), lambda: v == const(),
             lambda: Or(*[v == const() for _ in range(rng.randrange(2, 5))]),
             lambda: ULT(const(), v), lambda: ULE(v, const()),
             lambda: a + b == const(), lambda: ULT(a * b ^ v, const())][k]()
        return Not(c) if rng.random() < 0.3 else c

    cs = [atom() for _ in range(rng.randrange(2, 7))]
    return ctx, [c for c in cs if not isinstance(c, bool)]


def family(seed: int, n: int):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        ctx, cs = random_conjunction(rng)
        if cs:
            out.append((ctx, cs))
    return out


def models(ctx, cs):
    """Every satisfying assignment {name: value} of the 4-bit conjunction, by the oracle."""
    tapes = [ctx.b.finish(c.node).nodes for c in cs]  # conjunct by conjunct: the first false ends
    names = sorted(ctx.b.var_index, key=ctx.b.var_index.get)
    pool = ctx.b.pool.values
    out = []
    for vals in itertools.product(range(16), repeat=3):
        env = dict(zip(NAMES, vals))
        row = [env.get(n, 0) for n in names]
        if all(E.evaluate(t, pool, row) for t in tapes):
            out.append(env)
    return out


_TRUTH = {}


def truth(seed: int, n: int):
    """[(context, constraints, models)] of family(seed, n), computed once per process and shared
    by the tests that need it (left unchanged by them)."""
    if (seed, n) not in _TRUTH:
        _TRUTH[seed, n] = [(ctx, cs, models(ctx, cs)) for ctx, cs in family(seed, n)]
    return _TRUTH[seed, n]


def holds(ctx, cs, values) -> bool:
    """Whether {name: value} (missing names read 0) satisfies the conjunction (the oracle)."""
    tape = ctx.b.finish(And(*cs).node)
    names = sorted(ctx.b.var_index, key=ctx.b.var_index.get)
    return bool(E.evaluate(tape.nodes, ctx.b.pool.values, [values.get(n, 0) for n in names]))


def _f(x):
    """Arithmetic no syntactic refutation reads through: injective on 256-bit words."""
    return x * symbol_factory.BitVecVal(3, 256) + symbol_factory.BitVecVal(7, 256)


def actor_queries():
    """(context, {name: constraints}) over 256-bit columns:
    ``unsat``  the sender among the three actors, and f(sender) != f(A) for each actor A;
    ``sat``    the same without the last disequality (only SOMEGUY is left);
    ``mixed``  ``sat`` plus a free 256-bit group (bounds on ``amount`` the guided rounds meet)."""
    ctx = smt.set_context(smt.Context())
    sender = symbol_factory.BitVecSym("sender_1", 256)
    amount = symbol_factory.BitVecSym("amount", 256)
    actors = [symbol_factory.BitVecVal(a, 256) for a in (CREATOR, ATTACKER, SOMEGUY)]
    ne = [Not(_f(sender) == _f(a)) for a in actors]
    base = [sender_is_actor(sender)]
    free = [UGT(amount, symbol_factory.BitVecVal(1 << 200, 256)),
            ULT(amount + symbol_factory.BitVecVal(5, 256), symbol_factory.BitVecVal(1 << 220, 256))]
    return ctx, {"unsat": base + ne, "sat": base + ne[:2], "mixed": base + ne[:2] + free}
