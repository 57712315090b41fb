"""Sieve(spares=K, batch_spares=True) on the CPU stand-ins (tests/fake_hits_many.py): solve_many's
batched first rounds list hits and try the ancestors' rows, so on Sieves created alike it returns
what solve() returns on the same list in order -- witnesses with their spares, indices, rounds,
last_rounds, the stats integers, the spare counters and both stores.  Without the flag nothing
calls the batched listing and solve_many behaves as before; a batch the library refuses is answered
one by one."""
import pytest

from mythril_amd import native
from mythril_amd.sieve import Sieve
from tests import fake_hits_many, spares_cases as SC, test_sieve_trace as T

K = SC.K
KW = dict(rows=256, budget_s=600.0, seed=SC.SEED, spares=K)  # the stand-in is slow: no budget cut
STATS = ("queries", "hits", "misses", "rounds", "rows")
SPARE_COUNTERS = ("spare_rows", "spare_hits")


def _jumpi(name):
    ctx, parent, children = SC.CASES[name]()
    qs = [[c.node for c in cs] for cs in SC.sequence(parent, children, "jumpi")]
    return [ctx.b] * len(qs), qs


def _levels(*names):
    """Sequences of tests/test_sieve_trace.py's WORKLOAD, interleaved level by level (the first
    query of every sequence, then the second of each, ...): siblings of different paths share
    batches."""
    seqs = T.build([(n, make) for n, make in T.WORKLOAD if n in names])
    assert len(seqs) == len(names)
    bs, qs = [], []
    for level in range(max(len(q) for _, q in seqs)):
        for b, q in seqs:
            if level < len(q):
                bs.append(b)
                qs.append(q[level])
    return bs, qs


LISTS = {
    "one_group": lambda: _jumpi("one_group"),
    "two_groups": lambda: _jumpi("two_groups"),
    "jumpi_pair": lambda: _levels("one_group", "two_groups"),
    "mixed": lambda: _levels("one_group", "incremental", "selector", "two_groups"),
    "planted": lambda: _levels("planted_laser", "owner_check", "one_group"),
}
JUMPI = ("one_group", "two_groups", "jumpi_pair")


def _witness(w):
    return None if w is None else (sorted(w.values.items()), w.index, w.rounds, w.repaired,
                                   w.spares)


def _state(s):
    return dict(stats={k: getattr(s.stats, k) for k in STATS},
                spare={k: s.stats.extra.get(k) for k in SPARE_COUNTERS},
                witnesses=list(s.witnesses.items()),
                spare_witnesses=list(s.spare_witnesses.items()))


def sequential(bs, qs, **kw):
    s = Sieve(**dict(KW, **kw))
    try:
        recs = []
        for b, q in zip(bs, qs):
            w = s.solve(b, q, key=tuple(q))
            recs.append((_witness(w), dict(s.last_rounds), s.last_miss is not None))
        return recs, _state(s), dict(s.stats.extra)
    finally:
        s.close()


def batched(bs, qs, **kw):
    s = Sieve(**dict(KW, **kw))
    try:
        got = s.solve_many(bs, qs, keys=[tuple(q) for q in qs])
        assert all(r["error"] is None for r in s.last_many), s.last_many
        recs = [(_witness(w), dict(r["rounds"]), r["miss"] is not None)
                for w, r in zip(got, s.last_many)]
        return recs, _state(s), dict(s.stats.extra)
    finally:
        s.close()


@pytest.fixture(scope="module")
def lists():
    return {name: make() for name, make in LISTS.items()}


@pytest.fixture(scope="module")
def wanted(lists):
    """Every list through solve() in list order, once."""
    mp = pytest.MonkeyPatch()
    try:
        fake_hits_many.install(mp)
        return {name: sequential(*lists[name]) for name in LISTS}
    finally:
        mp.undo()


@pytest.mark.parametrize("name", list(LISTS))
def test_batched_spares_equal_sequential_solve(monkeypatch, lists, wanted, name):
    fake_hits_many.install(monkeypatch)
    want, want_state, want_extra = wanted[name]
    got, got_state, extra = batched(*lists[name], batch_spares=True)
    for i, (w, g) in enumerate(zip(want, got)):
        assert w == g, (name, i, w, g)
    assert got_state == want_state
    assert fake_hits_many.ROUNDS and min(fake_hits_many.ROUNDS) > 1
    assert extra["batched_rounds"] == sum(fake_hits_many.ROUNDS)
    assert "batch_refused" not in extra
    if name in JUMPI:  # both siblings share a batch and are answered by their parent's rows
        assert extra["batched_rounds"] >= 2 and extra["spare_hits"] >= 2
        assert want_extra["spare_hits"] == extra["spare_hits"]


def test_the_environment_switches_it_on(monkeypatch, lists, wanted):
    fake_hits_many.install(monkeypatch)
    monkeypatch.setenv("SIEVE_BATCH_SPARES", "1")
    got, got_state, _ = batched(*lists["one_group"])
    assert got == wanted["one_group"][0] and got_state == wanted["one_group"][1]
    assert fake_hits_many.ROUNDS == [2]
    # ... and only with spares
    s = Sieve(rows=256, batch_spares=True)
    assert s.spares == 0 and not s.batch_spares
    s.close()


@pytest.mark.parametrize("name", list(LISTS))
def test_without_the_flag_nothing_calls_the_batched_listing(monkeypatch, lists, name):
    """batch_spares=False is the behaviour before the flag: the batch is native.query_round_many's,
    a query whose first round it ran stores no spares, and the result is what a Sieve made without
    the keyword gives."""
    fake_hits_many.install(monkeypatch)

    def boom(ctx, jobs):
        raise AssertionError("query_round_hits_many called without batch_spares")

    monkeypatch.setattr(native, "query_round_hits_many", boom)
    monkeypatch.delenv("SIEVE_BATCH_SPARES", raising=False)
    bs, qs = lists[name]
    off = batched(bs, qs, batch_spares=False)
    assert off == batched(bs, qs)
    assert off[2]["batched_rounds"] >= 2
    # the queries of a batch: the runs of the list between two sequential first rounds
    s = Sieve(**KW)
    try:
        got = s.solve_many(bs, qs, keys=[tuple(q) for q in qs])
        batched_hits = [w for w, r in zip(got, s.last_many)
                        if w is not None and "spares" not in r["rounds"]]
        assert batched_hits and all(w.spares == [] for w in batched_hits)
    finally:
        s.close()


@pytest.mark.parametrize("name", ["one_group", "mixed"])
def test_a_refused_batch_is_answered_one_by_one(monkeypatch, lists, wanted, name):
    fake_hits_many.install(monkeypatch)
    calls = []

    def refuse(ctx, jobs):
        calls.append(len(jobs))
        raise native.Unsupported(native.MH_E_UNSUPPORTED,
                                 "mh_query_round_hits_many: job 0: a shape the batch refuses")

    monkeypatch.setattr(native, "query_round_hits_many", refuse)
    want, want_state, _ = wanted[name]
    got, got_state, extra = batched(*lists[name], batch_spares=True)
    assert got == want and got_state == want_state
    assert calls and extra["batch_refused"] == len(calls) and "batched_rounds" not in extra


def test_siblings_pack_their_ancestors_rows_once(monkeypatch, lists):
    """Two siblings of one batch share the limbs of their ancestor's rows (one array), and the
    values are what each would have packed alone."""
    import numpy as np

    fake_hits_many.install(monkeypatch)
    seen = []
    inner = fake_hits_many.fake_query_round_hits_many

    def spy(ctx, jobs):
        seen.append([j["spares"] for j in jobs])
        return inner(ctx, jobs)

    monkeypatch.setattr(native, "query_round_hits_many", spy)
    bs, qs = lists["one_group"]
    s = Sieve(**dict(KW, batch_spares=True))
    try:
        s.solve_many(bs, qs, keys=[tuple(q) for q in qs])
        (a, b), = seen
        assert a is not None and b is not None and a[1] is b[1]
        parent_key = tuple(qs[0])
        (column,) = s.witnesses[parent_key]  # one column: x
        alone = s._spare_rows(tuple(qs[1]), s.witnesses[parent_key], {column: 0}, s.first_rows)
        assert np.array_equal(alone[0], a[0]) and np.array_equal(alone[1], a[1])
        assert alone[1] is not a[1]
    finally:
        s.close()
