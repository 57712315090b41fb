"""frontend.configure(decide=...): what a query the sieve decided UNSAT becomes in get_model --
off: a miss like any other; True: UnsatError without the fallback; "audit": the fallback is still
asked and a model it returns is a dispute.  On the CPU stand-ins."""
import pytest

from mythril_amd import frontend
from mythril_amd.model import Model
from mythril_amd.support import SolverStatistics, UnsatError
from tests import decide_cases, fake_enumerate


@pytest.fixture
def front(monkeypatch):
    fake_enumerate.install(monkeypatch)
    monkeypatch.delenv("SIEVE_DECIDE", raising=False)
    frontend.reset()
    stats = SolverStatistics()
    saved = (stats.sieve_unsat, stats.sieve_unsat_disputed, stats.sieve_hits)
    stats.sieve_unsat = stats.sieve_unsat_disputed = 0
    calls = []

    def configure(answer="fallback", **kw):
        frontend.configure(rows=64, first_rows=64, budget_s=600.0, decide_rows=16)
        frontend.configure(fallback=lambda c, *a: calls.append(c) or answer, **kw)

    yield configure, calls, stats
    frontend.reset()
    stats.sieve_unsat, stats.sieve_unsat_disputed, stats.sieve_hits = saved


def test_off_the_decided_query_reaches_the_fallback(front):
    configure, calls, stats = front
    configure()
    ctx, qs = decide_cases.actor_queries()
    assert frontend.get_model(tuple(qs["unsat"])) == "fallback"
    assert len(calls) == 1 and stats.sieve_unsat == 0 and stats.sieve_unsat_disputed == 0
    assert frontend.sieve().stats.extra["decided_unsat"] == 1  # decided, and left a miss


def test_on_the_decided_query_raises_without_the_fallback(front):
    configure, calls, stats = front
    configure(decide=True)
    ctx, qs = decide_cases.actor_queries()
    with pytest.raises(UnsatError):
        frontend.get_model(tuple(qs["unsat"]))
    assert calls == [] and stats.sieve_unsat == 1 and stats.sieve_unsat_disputed == 0
    m = frontend.get_model(tuple(qs["sat"]))  # a witness from enumeration is a Model as ever
    assert isinstance(m, Model) and calls == [] and stats.sieve_unsat == 1
    for c in qs["sat"]:
        assert m.eval(c, model_completion=True) is True


def test_on_by_the_environment(front, monkeypatch):
    configure, calls, stats = front
    configure()
    monkeypatch.setenv("SIEVE_DECIDE", "1")
    ctx, qs = decide_cases.actor_queries()
    with pytest.raises(UnsatError):
        frontend.get_model(tuple(qs["unsat"]))
    assert calls == [] and stats.sieve_unsat == 1


def test_audit_asks_the_fallback_and_counts_a_dispute(front):
    configure, calls, stats = front
    configure(answer="a model", decide="audit")
    ctx, qs = decide_cases.actor_queries()
    assert frontend.get_model(tuple(qs["unsat"])) == "a model"
    assert len(calls) == 1 and stats.sieve_unsat == 1 and stats.sieve_unsat_disputed == 1


def test_audit_agreeing_fallback_is_no_dispute(front):
    configure, calls, stats = front

    def unsat(*a):
        calls.append(a[0])
        raise UnsatError

    frontend.configure(rows=64, first_rows=64, budget_s=600.0, decide_rows=16)
    frontend.configure(fallback=unsat, decide="audit")
    ctx, qs = decide_cases.actor_queries()
    with pytest.raises(UnsatError):
        frontend.get_model(tuple(qs["unsat"]))
    assert len(calls) == 1 and stats.sieve_unsat == 1 and stats.sieve_unsat_disputed == 0


def test_prefetched_decision_is_kept(front, monkeypatch):
    from tests import fake_batch

    configure, calls, stats = front
    fake_batch.install(monkeypatch)
    configure(decide=True)
    ctx, qs = decide_cases.actor_queries()
    assert frontend.prefetch([tuple(qs["unsat"]), tuple(qs["sat"])]) == 2
    with pytest.raises(UnsatError):
        frontend.get_model(tuple(qs["unsat"]))
    assert isinstance(frontend.get_model(tuple(qs["sat"])), Model)
    assert calls == [] and stats.sieve_unsat == 1


def test_bad_mode_is_refused(front):
    with pytest.raises(ValueError):
        frontend.configure(decide="maybe")
