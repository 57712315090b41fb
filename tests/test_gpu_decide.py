"""The decision step on an MI355X: tests/test_decide.py's verdict test with the device doing the
enumeration and the runs (Sieve with the native host stages), the hand-built 256-bit actor
queries, and get_model with decide=True."""
import pytest

from mythril_amd import frontend
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve
from mythril_amd.support import SolverStatistics, UnsatError
from tests import decide_cases
from tests.laser_like import SOMEGUY
from tests.test_reference_fixtures import holds_original

pytestmark = pytest.mark.gpu


def solve(s, ctx, cs):
    return s.solve(ctx.b, [c.node for c in cs])


def test_verdicts_equal_brute_force_on_the_random_family():
    """The first 60 queries of the 4-bit family (all eligible, at most 4096 rows; the brute force
    over more of them would take this test past a few seconds): a satisfiable one gets a model,
    an unsatisfiable one is decided UNSAT, never the other way round."""
    s = Sieve(budget_s=60.0, decide_rows=4096)
    try:
        n_sat = n_unsat = 0
        for i, (ctx, cs, sat) in enumerate(decide_cases.truth(decide_cases.SEED, 60)):
            before = s.stats.extra.get("native_unsupported", 0)
            w = solve(s, ctx, cs)
            if s.stats.extra.get("native_unsupported", 0) != before:
                assert not s.last_unsat
                continue
            if sat:
                assert w is not None and not s.last_unsat, i
                assert decide_cases.holds(ctx, cs, w.values), (i, w.values)
                n_sat += 1
            else:
                assert w is None and s.last_unsat, i
                n_unsat += 1
        assert n_sat >= 10 and n_unsat >= 10
        ex = s.stats.extra
        assert ex["decided_unsat"] == n_unsat
        assert not ex.get("decide_too_large") and not ex.get("decide_budget")
    finally:
        s.close()


def test_actor_queries():
    ctx, qs = decide_cases.actor_queries()
    s = Sieve(budget_s=60.0, decide_rows=16)
    try:
        assert solve(s, ctx, qs["unsat"]) is None and s.last_unsat
        assert s.stats.extra["decide_rows"] == 3
        w = solve(s, ctx, qs["sat"])
        assert w is not None and not s.last_unsat and w.values["sender_1"] == SOMEGUY
        assert holds_original(ctx, qs["sat"], w.schema, w.values)
        w = solve(s, ctx, qs["mixed"])
        assert w is not None and not s.last_unsat and w.values["sender_1"] == SOMEGUY
        assert holds_original(ctx, qs["mixed"], w.schema, w.values)
    finally:
        s.close()
    off = Sieve(budget_s=60.0)
    try:
        assert solve(off, ctx, qs["unsat"]) is None and not off.last_unsat
    finally:
        off.close()


def test_get_model_with_decide_on():
    """The UNSAT query raises without the fallback; the SAT one returns a certified Model."""
    stats = SolverStatistics()
    frontend.reset()
    calls = []
    try:
        frontend.configure(budget_s=60.0, decide_rows=16)
        frontend.configure(fallback=lambda c, *a: calls.append(c) or "fallback", decide=True,
                           certify=True)
        unsat0, hits0, rejected0 = stats.sieve_unsat, stats.sieve_hits, stats.sieve_rejected
        ctx, qs = decide_cases.actor_queries()
        with pytest.raises(UnsatError):
            frontend.get_model(tuple(qs["unsat"]))
        assert calls == [] and stats.sieve_unsat == unsat0 + 1
        m = frontend.get_model(tuple(qs["sat"]))
        assert isinstance(m, Model) and calls == []
        assert stats.sieve_hits == hits0 + 1 and stats.sieve_rejected == rejected0
        for c in qs["sat"]:
            assert m.eval(c, model_completion=True) is True
    finally:
        frontend.reset()


def test_enumeration_finds_the_smallest_row_in_windows():
    """tests/test_decide.py's window query with the same sieve options (the guided rows are the
    stand-in's bit for bit, so the round misses here as it does there): 256 rows in windows of
    the 64-row buffer, the witness is the smallest model."""
    from mythril_amd import smt
    from mythril_amd.smt import ULT, symbol_factory

    ctx = smt.set_context(smt.Context())
    x, y = symbol_factory.BitVecSym("x", 8), symbol_factory.BitVecSym("y", 8)
    c = lambda v: symbol_factory.BitVecVal(v, 8)  # noqa: E731
    cs = [ULT(x, c(16)), ULT(y, c(16)), x * x + y * c(5) == c(94), x * c(3) + y == c(30)]
    rows = [g for g in range(256) if ((g % 16) ** 2 + (g // 16) * 5) % 256 == 94
            and ((g % 16) * 3 + g // 16) % 256 == 30]
    s = Sieve(rows=64, first_rows=64, max_rounds=1, second_round="never", budget_s=60.0,
              decide_rows=256)
    try:
        w = solve(s, ctx, cs)
        assert w is not None and s.stats.extra.get("decided_sat") == 1
        assert w.index == rows[0]
        assert (w.values["x"], w.values["y"]) == (rows[0] % 16, rows[0] // 16)
        assert s.stats.extra["decide_rows"] == 64 * (rows[0] // 64 + 1)
    finally:
        s.close()
