"""The sieve's decision step (Sieve(decide_rows=...), DESIGN §6 "Decision by enumeration") on the
CPU stand-ins (tests/fake_device.py, tests/fake_enumerate.py): verdicts against brute force,
hand-built 256-bit queries, ineligible groups, undecided outcomes and refuted queries."""
from mythril_amd import native, smt
from mythril_amd.sieve import Sieve
from mythril_amd.smt import Not, ULT, symbol_factory
from tests import decide_cases, fake_enumerate
from tests.laser_like import SOMEGUY, hard_queries, queries
from tests.reference_cases import CASES, DIVERGENT
from tests.test_reference_fixtures import holds_original


def solve(s, ctx, cs):
    return s.solve(ctx.b, [c.node for c in cs])


def test_verdicts_equal_brute_force_on_the_random_family(monkeypatch):
    """decide_rows = 4096 covers every query of the 4-bit family: a satisfiable one gets a
    witness that is a model (the oracle), an unsatisfiable one is decided UNSAT -- never the
    other way round, and no eligible query is left a plain miss."""
    fake_enumerate.install(monkeypatch)
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=4096)
    n_sat = n_unsat = 0
    for i, (ctx, cs, sat) in enumerate(decide_cases.truth(decide_cases.SEED,
                                                          decide_cases.COUNT)):
        before = dict(s.stats.extra)
        try:
            w = solve(s, ctx, cs)
        except native.SieveError:
            continue
        ex = s.stats.extra
        if ex.get("native_unsupported", 0) != before.get("native_unsupported", 0):
            assert not s.last_unsat  # the Python host stages are never decided
            continue
        assert ex.get("decide_too_large", 0) == 0 and ex.get("decide_budget", 0) == 0
        assert ex.get("decide_ineligible", 0) == 0
        if sat:
            assert not s.last_unsat, (i, [str(c) for c in cs])
            assert w is not None, (i, [str(c) for c in cs])
            assert decide_cases.holds(ctx, cs, w.values), (i, w.values)
            n_sat += 1
        else:
            assert w is None and s.last_unsat, (i, [str(c) for c in cs])
            n_unsat += 1
    assert n_sat >= 20 and n_unsat >= 20
    assert s.stats.extra["decided_unsat"] == n_unsat
    assert s.stats.extra.get("decided_sat", 0) >= 1 and s.stats.extra["decide_rows"] > 0
    s.close()


def test_actor_queries(monkeypatch):
    """The sender among the three actors with f(sender) != f(A) for every actor: nothing the
    host refutes, three rows decide it.  One disequality fewer leaves SOMEGUY."""
    fake_enumerate.install(monkeypatch)
    ctx, qs = decide_cases.actor_queries()
    off = Sieve(rows=64, first_rows=64, budget_s=600.0)
    assert solve(off, ctx, qs["unsat"]) is None and not off.last_unsat
    assert "decided_unsat" not in off.stats.extra and off.stats.extra.get("refuted", 0) == 0
    off.close()
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=16)
    assert solve(s, ctx, qs["unsat"]) is None and s.last_unsat
    assert s.stats.extra["decided_unsat"] == 1 and s.stats.extra["decide_rows"] == 3
    assert s.stats.misses == 1  # (still a miss to a caller that ignores last_unsat)
    w = solve(s, ctx, qs["sat"])
    assert w is not None and not s.last_unsat
    assert w.values["sender_1"] == SOMEGUY
    assert holds_original(ctx, qs["sat"], w.schema, w.values)
    s.close()


def test_mixed_query_decides_the_finite_group_only(monkeypatch):
    """One finite group and one free 256-bit group: whichever the rounds leave unsolved, the
    free group is never enumerated (2^256 rows > decide_rows) and the answer is a model."""
    fake_enumerate.install(monkeypatch)
    ctx, qs = decide_cases.actor_queries()
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=16)
    w = solve(s, ctx, qs["mixed"])
    assert w is not None and not s.last_unsat
    assert w.values["sender_1"] == SOMEGUY and w.values["amount"] > (1 << 200)
    assert holds_original(ctx, qs["mixed"], w.schema, w.values)
    assert all(base + n <= 3 for base, n in fake_enumerate.WINDOWS)
    # the finite group empty, the free one satisfiable: UNSAT all the same
    ne = Not(symbol_factory.BitVecSym("sender_1", 256) * symbol_factory.BitVecVal(3, 256)
             + symbol_factory.BitVecVal(7, 256)
             == symbol_factory.BitVecVal((SOMEGUY * 3 + 7) % (1 << 256), 256))
    assert solve(s, ctx, qs["mixed"] + [ne]) is None and s.last_unsat
    s.close()


def test_windows_follow_the_buffer(monkeypatch):
    """A product larger than the buffer is enumerated in windows of its capacity, in order, up
    to the first window with a hit."""
    fake_enumerate.install(monkeypatch)
    ctx = smt.set_context(smt.Context())
    x, y = symbol_factory.BitVecSym("x", 8), symbol_factory.BitVecSym("y", 8)
    c = lambda v: symbol_factory.BitVecVal(v, 8)  # noqa: E731
    # 16 x 16 = 256 rows, x the fast digit; the smallest model by brute force (x = 7, y = 9 is
    # one: row 151)
    cs = [ULT(x, c(16)), ULT(y, c(16)), x * x + y * c(5) == c(94), x * c(3) + y == c(30)]
    rows = [g for g in range(256) if ((g % 16) ** 2 + (g // 16) * 5) % 256 == 94
            and ((g % 16) * 3 + g // 16) % 256 == 30]
    assert 151 in rows and rows[0] >= 64
    s = Sieve(rows=64, first_rows=64, max_rounds=1, second_round="never", budget_s=600.0,
              decide_rows=256)
    w = solve(s, ctx, cs)
    assert w is not None and decide_cases.holds(ctx, cs, w.values)
    assert s.stats.extra.get("decided_sat") == 1  # (the guided round's 64 rows miss it)
    assert fake_enumerate.WINDOWS == [(b, 64) for b in range(0, rows[0] + 1, 64)]
    assert w.index == rows[0]
    assert (w.values["x"], w.values["y"]) == (rows[0] % 16, rows[0] // 16)
    s.close()


def test_keccak_groups_are_never_decided(monkeypatch):
    """Every reference outcome case keeps its outcome with decide_rows set, and the
    expected-UNSAT keccak cases still end as plain misses: a group that touches keccak is
    ineligible whatever its domains."""
    fake_enumerate.install(monkeypatch)
    for case in CASES:
        ctx, cs = case.build()
        plain = Sieve(rows=64, first_rows=64, budget_s=600.0)
        s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=1 << 16)
        try:
            outcome = []
            for sv in (plain, s):
                try:
                    outcome.append(solve(sv, ctx, cs) is not None)
                except Exception as e:  # noqa: BLE001 - an unsupported case stays unsupported
                    outcome.append(type(e).__name__)
            assert outcome[0] == outcome[1], case.name
            if s.last_unsat:
                assert case.expected == "unsat" and case.name not in DIVERGENT, case.name
            if "keccak" in case.name:
                assert not s.last_unsat, case.name
        finally:
            plain.close()
            s.close()


def test_keccak_reading_query_is_ineligible(monkeypatch):
    """The LASER-shaped queries that read keccak (a mapping slot, an aliased one): whatever the
    rounds answer, nothing about them is decided with the decision step on."""
    fake_enumerate.install(monkeypatch)
    ctx, qs = queries()
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=1 << 16)
    for name in ("keccak_mapping", "keccak_alias"):
        w = solve(s, ctx, dict(qs)[name])
        assert not s.last_unsat, name
        assert "decided_sat" not in s.stats.extra and "decided_unsat" not in s.stats.extra
    s.close()


def test_undecided_outcomes(monkeypatch):
    """rows > decide_rows leaves the group undecided, and so does a spent budget: a window that
    would start after it is not started, and the group does not count as empty."""
    fake_enumerate.install(monkeypatch)
    ctx, qs = decide_cases.actor_queries()
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=2)
    assert solve(s, ctx, qs["unsat"]) is None and not s.last_unsat
    assert s.stats.extra["decide_too_large"] == 1 and "decide_rows" not in s.stats.extra
    s.close()
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=16)
    import time

    real = time.perf_counter
    # the clock jumps an hour once the first round has run: the budget is spent before the
    # decision step's first window
    monkeypatch.setattr(native, "query_round", _then_jump(native.query_round, monkeypatch, real))
    assert solve(s, ctx, qs["unsat"]) is None and not s.last_unsat
    assert s.stats.extra.get("decide_budget") == 1 and "decided_unsat" not in s.stats.extra
    assert fake_enumerate.WINDOWS == []
    s.close()


def _then_jump(fn, monkeypatch, real):
    def run(*a, **kw):
        out = fn(*a, **kw)
        import mythril_amd.sieve as sieve_mod

        monkeypatch.setattr(sieve_mod.time, "perf_counter", lambda: real() + 3600.0)
        return out
    return run


def test_refuted_queries(monkeypatch):
    """An eligible query the host refutes sets last_unsat without a device round; a refuted
    query with a keccak table does not."""
    fake_enumerate.install(monkeypatch)
    ctx, qs = hard_queries()
    s = Sieve(rows=64, first_rows=64, budget_s=600.0, decide_rows=16)
    r0 = s.stats.rounds
    assert solve(s, ctx, dict(qs)["overflow_unsat"]) is None
    assert s.last_unsat and s.stats.rounds == r0 and s.stats.extra["decided_unsat"] == 1
    off = Sieve(rows=64, first_rows=64, budget_s=600.0)
    assert solve(off, ctx, dict(qs)["overflow_unsat"]) is None and not off.last_unsat
    off.close()
    # the same contradiction beside a keccak application: refuted, but not ours to call UNSAT
    from tests.laser_like import KeccakManager

    ctx = smt.set_context(smt.Context())
    km = KeccakManager()
    x = symbol_factory.BitVecSym("x", 256)
    h, cond = km.create(x)
    one, two = symbol_factory.BitVecVal(1, 256), symbol_factory.BitVecVal(2, 256)
    cs = [cond, x == one, x == two, ULT(h, symbol_factory.BitVecVal(1 << 255, 256))]
    assert solve(s, ctx, cs) is None
    assert s.stats.extra.get("refuted", 0) == 2 and not s.last_unsat
    assert s.stats.extra["decided_unsat"] == 1
    s.close()
