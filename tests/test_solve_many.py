"""Sieve.solve_many's host logic on the CPU (tests/fake_batch.py stands in for the device): on
Sieves created alike it returns, query for query, what solve() returns on the list in order --
the same witness values, index and rounds -- advances the same counters and leaves the same
witness store; a child listed after its parent waits for it; duplicates, refuted and unsupported
queries and a spent budget are handled per query."""
import pytest

from mythril_amd import native
from mythril_amd.sieve import Sieve
from tests import fake_batch
from tests.laser_like import hard_queries, queries
from tests.planted import planted_path
from tests.test_gpu_frontend import _oracle_holds

KW = dict(rows=64, first_rows=64, budget_s=600.0)  # the CPU stand-in is slow: no budget cut
COUNTERS = ("queries", "rounds", "rows", "hits", "misses")


def same_witness(a, b):
    if a is None or b is None:
        return a is None and b is None
    return (a.values, a.index, a.rounds, a.repaired) == (b.values, b.index, b.rounds, b.repaired)


def both_ways(bs, qs, keys, **kw):
    """(sequential results, its sieve, its per-query (last_miss, last_rounds)), (solve_many's
    results, its sieve)."""
    seq = Sieve(**dict(KW, **kw))
    want, recs = [], []
    for b, q, k in zip(bs, qs, keys):
        want.append(seq.solve(b, q, key=k))
        recs.append((seq.last_miss, dict(seq.last_rounds)))
    many = Sieve(**dict(KW, **kw))
    got = many.solve_many(bs, qs, keys=keys)
    return (want, seq, recs), (got, many)


def assert_same(seq_side, many_side):
    (want, seq, recs), (got, many) = seq_side, many_side
    assert len(want) == len(got)
    for i, (w, g) in enumerate(zip(want, got)):
        assert same_witness(w, g), (i, w, g)
        miss, rounds = recs[i]
        r = many.last_many[i]
        assert r["error"] is None and r["rounds"] == rounds, (i, r, rounds)
        assert (r["miss"] is None) == (miss is None), i
        if miss is not None:
            assert r["miss"][0] == miss[0] and len(r["miss"]) == len(miss)
    for c in COUNTERS:
        assert getattr(seq.stats, c) == getattr(many.stats, c), c
    assert list(seq.witnesses.items()) == list(many.witnesses.items())


def test_equals_sequential_on_laser_shaped_queries(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    roots = [[c.node for c in cs] for _, cs in qs]
    keys = [tuple(r) for r in roots]
    seq_side, many_side = both_ways([ctx.b] * len(roots), roots, keys)
    assert_same(seq_side, many_side)
    got, many = many_side
    assert fake_batch.ROUNDS and max(fake_batch.ROUNDS) > 1  # first rounds really shared a batch
    assert many.stats.extra["batched_rounds"] == sum(fake_batch.ROUNDS)
    for (name, cs), w in zip(qs, got):
        if name.startswith("unsat"):
            assert w is None, name
        else:
            assert w is not None and _oracle_holds(ctx, cs, w.schema, w.values), name
    many.close()
    seq_side[1].close()


def _interleaved(n, seeds=(3, 4)):
    """Prefixes of two planted LASER paths in BFS order: A1 B1 A2 B2 ..., keyed as get_model keys
    them (a child's parent key is the previous query of its own path)."""
    paths = [planted_path("laser", s, n) for s in seeds]
    bs, qs, keys = [], [], []
    for k in range(1, n + 1):
        for ctx, cs, _, _ in paths:
            if k <= len(cs):
                nodes = [c.node for c in cs[:k]]
                bs.append(ctx.b)
                qs.append(nodes)
                keys.append(tuple(nodes))
    return bs, qs, keys


def test_equals_sequential_on_interleaved_planted_prefixes(monkeypatch):
    fake_batch.install(monkeypatch)
    bs, qs, keys = _interleaved(6)
    seq_side, many_side = both_ways(bs, qs, keys)
    assert_same(seq_side, many_side)
    # every level's two queries share a batch; a child never shares one with its parent
    assert fake_batch.ROUNDS and set(fake_batch.ROUNDS) == {2}
    assert sum(w is not None for w in many_side[0]) >= len(qs) // 2
    many_side[1].close()
    seq_side[1].close()


def test_child_listed_after_its_parent_waits_for_it(monkeypatch):
    """[parent, child, other]: the child is harvested under the parent's witness, as in
    sequential solve (its guide is built from it), so it cannot be staged before the parent has
    finished: the list runs as [parent] then [child, other]."""
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    cs = dict(qs)["killbilly"]
    other = [c.node for c in dict(qs)["selector"]]
    nodes = [c.node for c in cs]
    k = len(nodes) - 1
    roots = [nodes[:k], nodes, other]
    keys = [tuple(r) for r in roots]
    seen = []
    orig = Sieve._ancestor

    def spy(self, key, root_ends):
        w, n = orig(self, key, root_ends)
        seen.append((key, w is not None))
        return w, n

    monkeypatch.setattr(Sieve, "_ancestor", spy)
    seq_side, many_side = both_ways([ctx.b] * 3, roots, keys)
    assert_same(seq_side, many_side)
    assert fake_batch.ROUNDS == [2]  # the child and the unrelated query
    got, many = many_side
    assert got[0] is not None
    # both sieves' child stages found the parent's witness in the store
    assert [hit for key, hit in seen if key == keys[1]] == [True, True]
    many.close()
    seq_side[1].close()


def test_duplicates_are_solved_once(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    a = [c.node for c in dict(qs)["selector"]]
    b = [c.node for c in dict(qs)["owner_check"]]
    s = Sieve(**KW)
    got = s.solve_many(ctx.b, [a, b, a, a], keys=[tuple(a), tuple(b), tuple(a), tuple(a)])
    assert got[0] is not None and got[2] is got[0] and got[3] is got[0]
    assert s.stats.queries == 4 and s.stats.rounds == 2 and s.stats.hits == 4
    assert fake_batch.ROUNDS == [2]
    assert s.last_many[2]["rounds"] == s.last_many[0]["rounds"]
    # the numbers still go by list position: the next query is number 5
    w = s.solve(ctx.b, b, key=tuple(b))
    assert w is not None and w.index >> 24 == 5
    s.close()


def test_refuted_and_unsupported_queries_do_not_fail_the_list(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = hard_queries()
    refuted = [c.node for c in dict(qs)["killbilly_unsat"]]
    unsat = [c.node for c in dict(qs)["ether_thief_unsat"]]
    ctx2, qs2 = queries()  # a builder of its own for the satisfiable one
    sat = [c.node for c in dict(qs2)["selector"]]
    s = Sieve(**KW)
    boom = native.Unsupported(native.MH_E_UNSUPPORTED, "a shape the device path does not cover")
    orig = Sieve._stage

    def stage(self, b, roots, key, keccak_reads, qno, base_schema=None):
        if list(roots) == unsat[:2]:
            raise boom
        return orig(self, b, roots, key, keccak_reads, qno, base_schema)

    monkeypatch.setattr(Sieve, "_stage", stage)
    roots = [refuted, unsat[:2], unsat, sat]
    got = s.solve_many([ctx.b, ctx.b, ctx.b, ctx2.b], roots, keys=[tuple(r) for r in roots])
    assert got[0] is None and got[1] is None and got[2] is None
    assert s.stats.extra.get("refuted") == 1
    rec = s.last_many
    assert rec[0]["error"] is None and rec[0]["miss"] is None and rec[0]["rounds"] == {}
    assert rec[1]["error"] is boom
    assert rec[2]["error"] is None and rec[2]["miss"][0] == tuple(unsat)
    assert rec[2]["rounds"]["rounds"] == 1
    assert got[3] is not None and rec[3]["error"] is None
    # the refuted query ran no round, the unsupported one is no miss (solve() would have raised)
    assert s.stats.queries == 4 and s.stats.misses == 2 and s.stats.hits == 1
    assert fake_batch.ROUNDS == [2]
    s.close()


def test_budget_is_the_whole_lists(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    roots = [[c.node for c in cs] for _, cs in qs][:4]
    s = Sieve(**KW)
    assert s.solve_many(ctx.b, roots, budget_s=0.0) == [None] * 4
    assert s.stats.queries == 4 and s.stats.misses == 4 and s.stats.rounds == 0
    assert fake_batch.ROUNDS == []
    # spent while the list is being staged: the queries not started are misses, those started
    # are finished or missed by their own rounds' budget checks
    import time as _time

    t = [0.0]
    monkeypatch.setattr(_time, "perf_counter", lambda: t[0])
    orig = Sieve._stage

    def slow_stage(self, *a, **kw):
        t[0] += 10.0
        return orig(self, *a, **kw)

    monkeypatch.setattr(Sieve, "_stage", slow_stage)
    s2 = Sieve(**KW)
    got = s2.solve_many(ctx.b, roots, budget_s=15.0)
    assert s2.stats.queries == 4
    assert got[2] is None and got[3] is None  # never staged
    assert s2.stats.misses >= 2 and s2.stats.hits + s2.stats.misses == 4
    s.close()
    s2.close()


def test_empty_list_and_bad_arguments(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    s = Sieve(**KW)
    assert s.solve_many(ctx.b, []) == [] and s.stats.queries == 0
    with pytest.raises(ValueError):
        s.solve_many(ctx.b, [[1]], keys=[None, None])
    s.close()


def test_repair_straight_after_a_batched_round_repairs_the_same_rows(monkeypatch):
    """The chain queries miss their first round and have no later one (max_rounds=1): sequential
    solve() hands them to repair with the first round's rows in the sieve's own buffer; after a
    batched round those rows are regenerated there, so repair scores, selects and mutates the
    same rows and finds the same witness."""
    from tests import repair_ref
    from tests.repair_cases import chain_query

    repair_ref.install(monkeypatch)
    monkeypatch.setattr(native, "query_round_many", fake_batch.fake_query_round_many)
    del fake_batch.ROUNDS[:]
    kw = dict(rows=256, first_rows=256, max_rounds=1, keccak_second_chance=False,
              repair_rounds=8, repair_elites=8, repair_children=8)
    chains = [chain_query(6), chain_query(5)]
    bs = [ctx.b for ctx, _ in chains]
    qs = [[c.node for c in cs] for _, cs in chains]
    keys = [tuple(q) for q in qs]
    seq_side, many_side = both_ways(bs, qs, keys, **kw)
    assert_same(seq_side, many_side)
    (want, seq, _), (got, many) = seq_side, many_side
    assert fake_batch.ROUNDS == [2]
    assert got[0] is not None and got[0].repaired
    assert many.stats.extra["repair_regenerated"] == 2
    for k in ("repair_tries", "repair_iters", "repair_hits"):
        assert many.stats.extra.get(k) == seq.stats.extra.get(k), k
    many.close()
    seq.close()
