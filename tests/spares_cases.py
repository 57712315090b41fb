"""The spare-witness policy cases (DESIGN §6 "Spare witnesses"), shared by tests/test_spares.py
(the CPU stand-in) and tests/test_gpu_spares.py (the device): a parent query and the two successors
of a JUMPI on it, run in LASER order (the path: parent, then one child) and in JUMPI order (parent,
then both siblings back to back, as svm.py asks them)."""
from mythril_amd import smt
from mythril_amd.smt import Not, ULT, symbol_factory
from tests import hits_ref
from tests.test_reference_fixtures import holds_original

SEED = 0x5EED5EED  # the parent's spares hold both parities under it (asserted by the tests)
K = 8


def _bv(v):
    return symbol_factory.BitVecVal(v, 256)


def one_group():
    """parent ULT(x, 1000); children x & 1 == 0 and its negation."""
    ctx = smt.set_context(smt.Context())
    x = symbol_factory.BitVecSym("x", 256)
    even = (x & 1) == 0
    return ctx, [ULT(x, _bv(1000))], (even, Not(even))


def two_groups():
    """The same over two variable-disjoint groups: the children's condition reads x only."""
    ctx = smt.set_context(smt.Context())
    x = symbol_factory.BitVecSym("x", 256)
    y = symbol_factory.BitVecSym("y", 256)
    even = (x & 1) == 0
    return ctx, [ULT(x, _bv(1000)), ULT(y, _bv(1000))], (even, Not(even))


CASES = {"one_group": one_group, "two_groups": two_groups}


def sequence(parent, children, order):
    """The queries of a run, as constraint lists."""
    qs = [parent[:i] for i in range(1, len(parent) + 1)]
    qs.append(parent + [children[0]])
    if order == "jumpi":
        qs.append(parent + [children[1]])
    return qs


def jumpi_path(cs):
    """A path's queries in JUMPI order: at every constraint both successors, the taken one first."""
    qs = []
    for i, c in enumerate(cs):
        qs.append(cs[:i] + [c])
        qs.append(cs[:i] + [Not(c)])
    return qs


def run(s, ctx, qs):
    """Every query through Sieve.solve, keyed as get_model keys it: per query (constraints,
    witness or None, its global_base, the spares part of last_rounds, stats.rounds after it)."""
    out = []
    for cs in qs:
        nodes = [c.node for c in cs]
        w = s.solve(ctx.b, nodes, key=tuple(nodes))
        out.append((cs, w, s.stats.queries << 24, s.last_rounds.get("spares", 0),
                    s.last_rounds.get("spare_hit", 0), s.stats.rounds))
    return out


def summary(records):
    """What the device and the stand-in must agree on."""
    return [(None if w is None else (sorted(w.values.items()), w.index, w.rounds, w.spares),
             n_sp, hit, rounds) for _, w, _, n_sp, hit, rounds in records]


def first_satisfying(ctx, cs, schema, rows, base):
    """The global index of the first of the ancestor's `rows` (tried as rows base.. of the round)
    that is a model of `cs`, from the oracle's Bools through hits_ref's select."""
    bools = [holds_original(ctx, cs, schema, dict(r)) for r in rows]
    hits, n, _ = hits_ref.select(hits_ref.pack_masks(bools), len(bools), 1, base)
    return hits[0] if n else None
