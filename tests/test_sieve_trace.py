"""The sieve driver's whole trace on the CPU stand-ins, against digests recorded before the driver
was last restructured (tests/golden/sieve_trace.json): for each of four configurations on its
matching stand-in, a fixed list of query sequences is solved in order with keys, and per query the
witness (values, index, rounds, repaired, spares), last_rounds, whether last_miss is set,
last_unsat and the exception type are recorded, then the stats counters and every key of
stats.extra; the same queries go through solve_many (tests/fake_batch.py) and last_many is
recorded likewise.  No wall-clock field is recorded; the stand-ins are deterministic, so the
SHA-256 of each trace is compared for equality.  The test also asserts that the workload reaches
every opt-in step of the driver (COVERED), so it cannot silently stop covering one.

To record the file again (only at a commit whose driver is the reference):
    python -m tests.test_sieve_trace tests/golden/sieve_trace.json
"""
import hashlib
import json
import os
import sys

import pytest

from mythril_amd import smt
from mythril_amd.sieve import Sieve
from mythril_amd.smt import ULT, symbol_factory
from tests import (decide_cases, fake_batch, fake_device, fake_enumerate, fake_hits, repair_ref,
                   spares_cases)
from tests.laser_like import hard_queries, queries
from tests.planted import planted_path
from tests.repair_cases import chain_query

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sieve_trace.json")

BASE = dict(rows=256, budget_s=600)  # the stand-ins are slow: no budget cut
CONFIGS = {
    "default": ({}, fake_device),
    "spares": (dict(spares=8), fake_hits),
    "repair": (dict(repair_rounds=2), repair_ref),
    "decide": (dict(decide_rows=1 << 16), fake_enumerate),
}
# counters of stats.extra that must be non-zero in at least one configuration
COVERED = ("inc_rounds", "keccak2_tries", "round2_skipped", "refuted", "spare_hits",
           "repair_iters", "repair_hits", "decide_rows", "decided_sat", "decided_unsat",
           "batched_rounds")
STATS = ("queries", "hits", "misses", "rounds", "rows")


def _prefixes(cs, last=None):
    """A path's queries in LASER order: every prefix, or the `last` longest ones."""
    return [cs[:k] for k in range(1, len(cs) + 1)][-(last or len(cs)):]


def _pinned_keccak():
    from tests.test_sieve_solve import _pinned_keccak_query

    ctx, cs = _pinned_keccak_query()
    return ctx, _prefixes(cs, 2)


def _laser(name, last=None, hard=False):
    def build():
        ctx, qs = (hard_queries if hard else queries)()
        return ctx, _prefixes(dict(qs)[name], last)
    return build


def _spares(name):
    def build():
        ctx, parent, children = spares_cases.CASES[name]()
        return ctx, spares_cases.sequence(parent, children, "jumpi")
    return build


def _actors():
    ctx, qs = decide_cases.actor_queries()
    return ctx, [qs["unsat"], qs["sat"], qs["mixed"]]


def _family(i):
    def build():
        ctx, cs = decide_cases.family(decide_cases.SEED, i + 1)[i]
        return ctx, [cs]
    return build


def _chain(m):
    def build():
        ctx, cs = chain_query(m)
        return ctx, [cs]
    return build


def _incremental():
    """A parent the first round answers, then two children whose first round solves the parent's
    groups but not the new conjunct's: each runs the incremental round under the parent's witness."""
    ctx = smt.set_context(smt.Context())
    x, y, z = (symbol_factory.BitVecSym(n, 256) for n in "xyz")
    v = lambda k: symbol_factory.BitVecVal(k, 256)  # noqa: E731
    parent = [x == v(5), ULT(y, v(1000))]
    return ctx, [parent, parent + [y * y == v(2)], parent + [y * v(3) + z == v(100)]]


def _planted(family, seed, n, upto, last):
    def build():
        ctx, cs, _, _ = planted_path(family, seed, n)
        return ctx, _prefixes(cs[:upto], last)
    return build


# the query sequences: (name, builder of (term context, [constraint lists in asking order]))
WORKLOAD = [
    # a keccak second chance with an incremental round under its parent's witness
    ("planted_laser", _planted("laser", 3, 12, 12, 3)),
    ("selector", _laser("selector")),
    ("owner_check", _laser("owner_check")),
    ("keccak_alias", _laser("keccak_alias")),
    ("pinned_keccak", _pinned_keccak),                     # the keccak second chance
    ("killbilly_unsat", _laser("killbilly_unsat", 1, True)),       # refuted, keccak table
    ("overflow_unsat", _laser("overflow_unsat", 1, True)),         # refuted, eligible
    ("one_group", _spares("one_group")),
    ("two_groups", _spares("two_groups")),
    ("actors", _actors),
    ("chain", _chain(6)),
    ("incremental", _incremental),
] + [("family%d" % i, _family(i)) for i in list(range(0, 24, 2)) + [147]]  # 147: decided SAT


def build(workload):
    """[(builder, [root node lists])] of a workload (each sequence in a term context of its own)."""
    out = []
    for _, make in workload:
        ctx, qs = make()
        out.append((ctx.b, [[c.node for c in cs] for cs in qs]))
    return out


def _witness(w):
    if w is None:
        return None
    return {"values": sorted(w.values.items()), "index": w.index, "rounds": w.rounds,
            "repaired": w.repaired, "spares": [sorted(x.items()) for x in w.spares]}


def _totals(s):
    return {"stats": {k: getattr(s.stats, k) for k in STATS},
            "extra": sorted(s.stats.extra.items())}


def _digest(trace):
    return hashlib.sha256(json.dumps(trace, sort_keys=True).encode()).hexdigest()


def sequential(kw, seqs):
    """(trace, stats integers, stats.extra) of every sequence solved query by query."""
    s = Sieve(**dict(BASE, **kw))
    try:
        recs = []
        for b, qs in seqs:
            for nodes in qs:
                w = err = None
                try:
                    w = s.solve(b, nodes, key=tuple(nodes))
                except Exception as e:  # noqa: BLE001 - what the front end falls back on
                    err = type(e).__name__
                recs.append({"witness": _witness(w), "rounds": dict(s.last_rounds),
                             "miss": s.last_miss is not None, "unsat": s.last_unsat,
                             "error": err})
        tot = _totals(s)
        return {"queries": recs, "totals": tot}, tot["stats"], dict(s.stats.extra)
    finally:
        s.close()


def many(kw, seqs):
    """The same queries through one solve_many call, level by level (the first query of every
    sequence, then the second of each, ...), so that queries share batches."""
    bs, roots = [], []
    for level in range(max(len(qs) for _, qs in seqs)):
        for b, qs in seqs:
            if level < len(qs):
                bs.append(b)
                roots.append(qs[level])
    s = Sieve(**dict(BASE, **kw))
    try:
        got = s.solve_many(bs, roots, keys=[tuple(r) for r in roots])
        recs = [{"witness": _witness(w), "rounds": dict(r["rounds"]),
                 "miss": r["miss"] is not None, "unsat": bool(r.get("unsat", False)),
                 "error": None if r["error"] is None else type(r["error"]).__name__}
                for w, r in zip(got, s.last_many)]
        tot = _totals(s)
        return {"queries": recs, "totals": tot}, tot["stats"], dict(s.stats.extra)
    finally:
        s.close()


def run(name, seqs, monkeypatch):
    """One configuration on its stand-in: ({sequential, many: digest, stats integers of the
    sequential run}, the union of both runs' stats.extra)."""
    kw, stand_in = CONFIGS[name]
    for k in [k for k in os.environ if k.startswith("SIEVE_")]:
        monkeypatch.delenv(k)
    fake_batch.install(monkeypatch)  # (first: the stand-in's own Context replaces fake_device's)
    stand_in.install(monkeypatch)
    seq_trace, stats, extra = sequential(kw, seqs)
    many_trace, _, extra_many = many(kw, seqs)
    for k, v in extra_many.items():
        extra[k] = extra.get(k, 0) + v
    return dict(stats, sequential=_digest(seq_trace), many=_digest(many_trace)), extra


@pytest.fixture(scope="module")
def traces():
    seqs = build(WORKLOAD)
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for name in CONFIGS:
            out[name] = run(name, seqs, mp)
            mp.undo()
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_trace_equals_the_recorded_one(traces, name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got, _ = traces[name]
    print(name, json.dumps(got))
    assert got == golden[name]


def test_workload_reaches_every_step(traces):
    seen = {}
    for _, extra in traces.values():
        for k, v in extra.items():
            seen[k] = seen.get(k, 0) + v
    print(sorted(seen.items()))
    assert [k for k in COVERED if not seen.get(k)] == []


if __name__ == "__main__":
    mp = pytest.MonkeyPatch()
    seqs = build(WORKLOAD)
    out = {}
    for name in CONFIGS:
        out[name], _ = run(name, seqs, mp)
        mp.undo()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
