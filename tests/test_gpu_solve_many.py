"""Sieve.solve_many and frontend.prefetch on an MI355X: on sieves created alike, solve_many
returns query for query what solve() returns on the list in order (witness values, index,
rounds), with the same counters and witness store -- LASER-shaped queries with their UNSAT
variants, and prefixes of planted paths interleaved in BFS order, once with the repair step on.
Every witness is checked by the oracle.  After prefetch, get_model answers from the parked
results without a device round."""
import pytest

from mythril_amd import frontend, native
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve
from mythril_amd.support import UnsatError
from tests.laser_like import hard_queries, queries
from tests.planted import planted_path
from tests.test_gpu_frontend import _oracle_holds
from tests.test_solve_many import COUNTERS, same_witness

pytestmark = pytest.mark.gpu

KW = dict(budget_s=60.0)  # no budget cut: the comparison is of what the rounds find


@pytest.fixture(autouse=True)
def _reset():
    frontend.reset()
    yield
    frontend.reset()


def _both_ways(ctxs, css, **kw):
    """solve() on the list in order and solve_many() on it, on two sieves created alike; the
    comparison; returns solve_many's witnesses and its sieve's stats."""
    bs = [c.b for c in ctxs]
    roots = [[t.node for t in cs] for cs in css]
    keys = [tuple(r) for r in roots]
    seq, many = Sieve(**dict(KW, **kw)), Sieve(**dict(KW, **kw))
    try:
        want, recs = [], []
        for b, r, k in zip(bs, roots, keys):
            want.append(seq.solve(b, r, key=k))
            recs.append((seq.last_miss, dict(seq.last_rounds)))
        got = many.solve_many(bs, roots, keys=keys)
        for i, (w, g) in enumerate(zip(want, got)):
            assert same_witness(w, g), (i, w, g)
            rec = many.last_many[i]
            assert rec["error"] is None and rec["rounds"] == recs[i][1], (i, rec, recs[i])
            assert (rec["miss"] is None) == (recs[i][0] is None), i
            if g is not None:
                assert _oracle_holds(ctxs[i], css[i], g.schema, g.values), i
        for c in COUNTERS:
            assert getattr(seq.stats, c) == getattr(many.stats, c), c
        assert list(seq.witnesses.items()) == list(many.witnesses.items())
        return got, many.stats
    finally:
        seq.close()
        many.close()


def test_laser_shaped_queries_and_unsat_variants(gpu_ctx):
    ctx, qs = queries()
    hctx, hqs = hard_queries()
    ctxs = [ctx] * len(qs) + [hctx] * len(hqs)
    css = [cs for _, cs in qs] + [cs for _, cs in hqs]
    names = [n for n, _ in qs] + [n for n, _ in hqs]
    got, stats = _both_ways(ctxs, css)
    assert stats.extra["batched_rounds"] >= len(qs)  # first rounds really shared submissions
    for name, w in zip(names, got):
        if "unsat" in name:
            assert w is None, name
    assert sum(w is not None for w in got) >= len(qs) - 2


def _interleaved(family, seeds, n):
    paths = [planted_path(family, s, n) for s in seeds]
    ctxs, css = [], []
    for k in range(1, n + 1):
        for ctx, cs, _, _ in paths:
            if k <= len(cs):
                ctxs.append(ctx)
                css.append(list(cs[:k]))
    return ctxs, css


@pytest.mark.parametrize("family,kw", [("laser", {}), ("random", {}),
                                       ("random", dict(repair_rounds=2))])
def test_interleaved_planted_prefixes(gpu_ctx, family, kw):
    ctxs, css = _interleaved(family, (5, 6), 8)
    got, stats = _both_ways(ctxs, css, **kw)
    assert stats.extra.get("batches", 0) >= 4 and len(got) >= 12
    assert any(w is not None for w in got)


def test_repair_straight_after_a_batched_round(gpu_ctx):
    """Chain queries (tests/repair_cases.py) miss their only round and go to repair at once:
    after a batched round its rows are regenerated into the buffer repair reads, and repair
    finds what it finds after sequential solve()."""
    from tests.repair_cases import chain_query

    kw = dict(rows=256, first_rows=256, max_rounds=1, keccak_second_chance=False,
              repair_rounds=8, repair_elites=8, repair_children=8)
    chains = [chain_query(6), chain_query(5), chain_query(4)]
    got, stats = _both_ways([ctx for ctx, _ in chains], [cs for _, cs in chains], **kw)
    assert stats.extra["repair_regenerated"] >= 1 and stats.extra["batches"] == 1
    assert any(w is not None and w.repaired for w in got)


def test_prefetch_then_get_model_runs_no_round(gpu_ctx):
    ctx, qs = queries()
    css = [tuple(cs) for _, cs in qs]
    calls = []
    frontend.configure(fallback=lambda c, *a: calls.append(c) or "fallback", **KW)
    parked = frontend.prefetch(css)
    assert parked == len(css)
    s = frontend.sieve()
    assert s.stats.extra["batched_rounds"] >= 2
    answered = 0
    for (name, cs), q in zip(qs, css):
        rounds, launches = s.stats.rounds, native.eval_launches(s.ctx)
        try:
            m = frontend.get_model(q)
        except UnsatError:
            m = None
        assert s.stats.rounds == rounds and native.eval_launches(s.ctx) == launches, name
        if isinstance(m, Model):
            assert _oracle_holds(ctx, cs, m.schema, m.values), name
            answered += 1
        else:
            assert m == "fallback", name
    assert answered >= len(css) - 2 and len(calls) == len(css) - answered
