"""The spare-witness policy of Sieve (Sieve(spares=K); DESIGN §6 "Spare witnesses") on the CPU
stand-in (tests/fake_hits.py): a solved query keeps further models beside its witness, a child's
first round tries its ancestor's witness and spares as its first rows, and with spares=0 nothing
of it runs.  tests/test_gpu_spares.py runs the same cases on the device."""
from collections import OrderedDict

import pytest

from mythril_amd import native
from mythril_amd.sieve import Sieve
from tests import fake_hits, spares_cases as SC
from tests.laser_like import queries
from tests.test_gpu_frontend import _oracle_holds
from tests.test_reference_fixtures import holds_original


def _sieve(spares, **kw):
    return Sieve(rows=256, budget_s=60.0, seed=SC.SEED, spares=spares, **kw)


def check_policy(make_sieve, name, order):
    """One case with spares on: every witness is a model; each child is answered at exactly the
    first of its ancestor's rows that satisfies it, group by group, with spare_hits counted.
    Returns the run's summary (the device test compares it with the stand-in's)."""
    ctx, parent, children = SC.CASES[name]()
    s = make_sieve(SC.K)
    try:
        recs = SC.run(s, ctx, SC.sequence(parent, children, order))
        pkey = tuple(c.node for c in parent)
        rows = [s.witnesses[pkey]] + s.spare_witnesses[pkey]
        # the precondition, on the reference alone: a spare of each parity
        assert len(rows) <= SC.K
        assert {r["x"] & 1 for r in rows[1:]} == {0, 1}, rows
        assert all(r["x"] < 1000 for r in rows)
        n_children = 0
        for cs, w, base, n_sp, hit, _ in recs:
            assert w is not None and holds_original(ctx, cs, w.schema, w.values)
            if len(cs) <= len(parent):
                if len(cs) == 1:  # (no ancestor)
                    assert n_sp == 0 and hit == 0
                continue
            n_children += 1
            child = cs[-1]
            assert n_sp == len(rows) and hit == 1
            # the group of x: its parent conjunct and the child's condition
            jx = SC.first_satisfying(ctx, [parent[0], child], w.schema, rows, base)
            assert jx is not None and w.values["x"] == rows[jx - base]["x"]
            if name == "two_groups":  # the group of y holds at row 0, the parent's model
                jy = SC.first_satisfying(ctx, [parent[1]], w.schema, rows, base)
                assert jy == base and w.values["y"] == rows[0]["y"]
                assert w.index == base
            else:
                assert w.index == jx
            assert w.rounds == 1
        assert n_children == (2 if order == "jumpi" else 1)
        assert s.stats.extra.get("spare_hits", 0) == sum(r[4] for r in recs) >= n_children
        assert s.stats.extra.get("spare_rows", 0) == sum(r[3] for r in recs)
        return SC.summary(recs)
    finally:
        s.close()


@pytest.mark.parametrize("order", ["laser", "jumpi"])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_children_are_answered_by_the_first_satisfying_spare(monkeypatch, name, order):
    fake_hits.install(monkeypatch)
    check_policy(_sieve, name, order)


def _raising(*a, **kw):
    raise AssertionError("a hit-listing entry point was called with spares=0")


@pytest.mark.parametrize("order", ["laser", "jumpi"])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_spares_off_takes_no_new_path(monkeypatch, name, order):
    """spares=0 with the three new native functions raising: the witnesses, indices and
    stats.rounds of a default Sieve."""
    fake_hits.install(monkeypatch)
    ctx, parent, children = SC.CASES[name]()
    qs = SC.sequence(parent, children, order)
    ref = Sieve(rows=256, budget_s=60.0, seed=SC.SEED)
    want = SC.summary(SC.run(ref, ctx, qs))
    monkeypatch.setattr(native, "run_hits", _raising)
    monkeypatch.setattr(native, "query_round_hits", _raising)
    monkeypatch.setattr(fake_hits.HitsAssign, "scatter", _raising)
    monkeypatch.setattr(native.Assignments, "scatter", _raising)
    s = _sieve(0)
    assert s.spares == 0
    assert SC.summary(SC.run(s, ctx, qs)) == want
    assert not s.spare_witnesses and "spare_rows" not in s.stats.extra
    assert all(w[0] is not None and w[0][3] == [] for w in want)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_spares_on_keeps_the_parent_and_answers_both_siblings(monkeypatch, name):
    """Hit 0 is the witness as without spares: the first query's witness, index and rounds are
    the default Sieve's; the parent keeps spares and both siblings are answered."""
    fake_hits.install(monkeypatch)
    ctx, parent, children = SC.CASES[name]()
    qs = SC.sequence(parent, children, "jumpi")
    off = SC.summary(SC.run(_sieve(0), ctx, qs))
    on = SC.summary(SC.run(_sieve(SC.K), ctx, qs))
    assert off[0][0][:3] == on[0][0][:3]  # (the path's first query has no ancestor to try)
    assert on[len(parent) - 1][0][3], "the parent keeps spares"
    assert all(r[0] is not None for r in on)


@pytest.mark.parametrize("name", ["balance", "owner_check"])
def test_laser_like_path_in_jumpi_order(monkeypatch, name):
    """A LASER-shaped path, both successors of every JUMPI: with spares on and off the same
    queries are answered, every witness is a model of its query, and a spare hit is one."""
    fake_hits.install(monkeypatch)
    ctx, qs = queries()
    path = SC.jumpi_path(dict(qs)[name])
    got = {}
    for sp in (0, SC.K):
        s = _sieve(sp)
        recs = SC.run(s, ctx, path)
        for cs, w, _, _, _, _ in recs:
            if w is not None:
                assert _oracle_holds(ctx, cs, w.schema, w.values)
                for r in w.spares:  # spares are models of the query's groups too
                    assert set(r) <= set(w.values)
        got[sp] = [w is not None for _, w, _, _, _, _ in recs]
        if sp:
            assert s.stats.extra.get("spare_rows", 0) >= 0
            assert s.stats.extra.get("spare_hits", 0) == sum(r[4] for r in recs)
    assert [a for a, b in zip(got[0], got[SC.K]) if a and not b] == []
    assert any(got[SC.K])


def test_env_overrides_and_clamps(monkeypatch):
    fake_hits.install(monkeypatch)
    monkeypatch.setenv("SIEVE_SPARES", "16")
    assert Sieve(rows=256).spares == 16
    monkeypatch.setenv("SIEVE_SPARES", "1000")
    assert Sieve(rows=256).spares == native.HITS_MAX
    monkeypatch.setenv("SIEVE_SPARES", "-3")
    assert Sieve(rows=256, spares=5).spares == 0
    monkeypatch.delenv("SIEVE_SPARES")
    assert Sieve(rows=256).spares == 0 and Sieve(rows=256, spares=99).spares == native.HITS_MAX


def test_no_stale_spares(monkeypatch):
    """forget, forget_witnesses, eviction and learn leave no spares behind."""
    from mythril_amd import frontend

    fake_hits.install(monkeypatch)
    ctx, parent, children = SC.one_group()
    s = _sieve(SC.K)
    pkey = tuple(c.node for c in parent)
    SC.run(s, ctx, [parent])
    assert s.spare_witnesses[pkey] and isinstance(s.spare_witnesses, OrderedDict)
    s.forget(pkey)
    assert pkey not in s.witnesses and pkey not in s.spare_witnesses
    # eviction takes the spares with the witness
    SC.run(s, ctx, [parent])
    s.max_witnesses = 1
    s._store(("other",), {"x": 1})
    assert list(s.witnesses) == [("other",)] and not s.spare_witnesses
    # a learnt model replaces the witness and stores no spares
    s.max_witnesses = 1 << 14
    SC.run(s, ctx, [parent])
    assert s.spare_witnesses[pkey]
    schema = s.solve(ctx.b, list(pkey), key=pkey).schema
    s.last_miss = (pkey, schema)
    assert s.learn(pkey, lambda col: 7) == 1
    assert s.witnesses[pkey] == {"x": 7} and pkey not in s.spare_witnesses
    # forget_witnesses clears both
    SC.run(s, ctx, [parent])
    assert s.spare_witnesses
    monkeypatch.setattr(frontend._tls, "sieve", s, raising=False)
    frontend.forget_witnesses()
    assert not s.witnesses and not s.spare_witnesses


def test_frontend_rejection_forgets_the_spares(monkeypatch):
    """A witness the certifier rejects leaves the sieve with its spares (frontend calls
    Sieve.forget where it dropped the witness)."""
    from mythril_amd import certify, frontend

    fake_hits.install(monkeypatch)
    frontend.reset()
    try:
        frontend.configure(rows=256, certify=True, fallback=lambda c, *a: "fallback",
                           sieve_kwargs={"spares": SC.K, "budget_s": 60.0})
        monkeypatch.setattr(frontend, "certify_resident_on", lambda: False)
        monkeypatch.setattr(certify, "certify", lambda m, terms: False)
        ctx, parent, _ = SC.one_group()
        assert frontend.get_model(tuple(parent)) == "fallback"
        s = frontend.sieve()
        assert s.spares == SC.K and s.stats.hits == 1
        assert not s.witnesses and not s.spare_witnesses
    finally:
        frontend.reset()
