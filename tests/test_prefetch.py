"""frontend.prefetch on the CPU (tests/fake_batch.py stands in for the device): answers parked by
one batched solve are used by get_model in place of a round of its own -- a hit through
certification and the verifier as any other, a miss straight to the fallback whose model is still
learnt -- the table is cleared with the configuration, objectives never look at it, and the plugin's
stop_sym_trans hook hands it the open states' constraints."""
import sys
import types

import pytest

from mythril_amd import frontend, plugin, smt
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve, Witness
from mythril_amd.smt import symbol_factory
from mythril_amd.support import SolverStatistics, UnsatError
from tests import fake_batch
from tests.laser_like import queries
from tests.test_sieve_solve import _Model, _Z3

KW = dict(rows=64, first_rows=64, budget_s=600.0)  # the CPU stand-in is slow: no budget cut
BVS, BVV = symbol_factory.BitVecSym, symbol_factory.BitVecVal


@pytest.fixture(autouse=True)
def _reset():
    frontend.reset()
    yield
    frontend.reset()


def _no_solve(monkeypatch):
    def solve(self, *a, **kw):
        raise AssertionError("get_model ran a round of its own")

    monkeypatch.setattr(Sieve, "solve", solve)


def test_parked_hits_answer_get_model_without_a_round(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    names = ["selector", "owner_check", "balance"]
    css = [tuple(dict(qs)[n]) for n in names]
    calls = []
    frontend.configure(fallback=lambda c, *a: calls.append(c) or "fallback", **KW)
    assert frontend.prefetch(css + [css[0]]) == 3  # the repeated query is parked once
    assert fake_batch.ROUNDS == [3]
    s = frontend.sieve()
    rounds, hits = s.stats.rounds, SolverStatistics().sieve_hits
    for cs in css:
        m = frontend.get_model(cs)
        assert isinstance(m, Model)
        for c in cs:
            assert m.eval(c, model_completion=True) is True
    assert s.stats.rounds == rounds and calls == []
    assert SolverStatistics().sieve_hits == hits + 3
    assert not frontend._parked()  # each answer is used once (get_model caches it itself)
    # a query that was not prefetched takes the ordinary path
    other = tuple(dict(qs)["selector_size"])
    assert isinstance(frontend.get_model(other), Model) and s.stats.rounds == rounds + 1


def test_python_bools_as_in_get_model(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    cs = tuple(dict(qs)["selector"])
    frontend.configure(fallback=lambda *a: "fallback", **KW)
    assert frontend.prefetch([(False,) + cs, (True,)]) == 0  # UNSAT without the sieve; nothing left
    assert frontend.prefetch([(True,) + cs]) == 1            # the bool is dropped: the same key
    _no_solve(monkeypatch)
    assert isinstance(frontend.get_model(cs), Model)


def test_parked_miss_goes_to_the_fallback_and_its_model_is_learnt(monkeypatch):
    import random

    fake_batch.install(monkeypatch)
    monkeypatch.setitem(sys.modules, "z3", _Z3)
    rng = random.Random(77)
    x0, y0 = rng.getrandbits(256) | 1, rng.getrandbits(256) | 1
    k = (x0 * y0) % (1 << 256)
    smt.set_context(smt.Context())
    x, y, z = (BVS(n, 256) for n in "xyz")
    c1 = x * y == BVV(k, 256)
    c2 = z == BVV(7, 256)
    calls = []

    def fallback(cs, mn, mx, enf):
        calls.append(len(cs))
        return _Model({"x": x0, "y": y0, "z": 0})

    frontend.configure(fallback=fallback, **KW)
    assert frontend.prefetch([(c1,)]) == 1
    s = frontend.sieve()
    assert s.stats.misses == 1 and s.last_miss is None  # parked, not left in the sieve
    rounds, misses = s.stats.rounds, SolverStatistics().sieve_misses
    real = Sieve.solve
    _no_solve(monkeypatch)
    assert isinstance(frontend.get_model((c1,)), _Model) and calls == [1]
    assert SolverStatistics().sieve_misses == misses + 1 and s.stats.rounds == rounds
    assert s.stats.extra.get("learnt") == 1
    # ... so the child is answered around the fallback's model, by the ordinary path
    monkeypatch.setattr(Sieve, "solve", real)
    m = frontend.get_model((c1, c2))
    assert isinstance(m, Model) and calls == [1]
    assert (m.values["x"], m.values["y"], m.values["z"]) == (x0, y0, 7)


def test_certification_rejects_a_bad_parked_witness(monkeypatch):
    from mythril_amd.lower import lower_query
    from mythril_amd.smt import Array
    from tests import fake_tables
    from tests.test_certify import _read_cols

    fake_tables.install(monkeypatch)
    ctx = smt.set_context(smt.Context())
    A = Array("A", 256, 256)
    i, j = BVS("i", 256), BVS("j", 256)
    cs = (A[i] == BVV(5, 256), A[j] == BVV(6, 256))
    _, schema = lower_query(ctx.b, [t.node for t in cs])
    ri, rj = _read_cols(schema, "read")
    values = {"i": 9, "j": 9, ri: 5, rj: 6}  # two reads at one index with unequal values

    def solve_many(self, b, queries, keys=None, budget_s=None):
        w = Witness(schema, dict(values), 0, 1)
        self.remember(keys[0], w)  # as solve_many does for a hit
        self.last_many = [dict(miss=None, rounds={"rounds": 1}, error=None)]
        return [w]

    monkeypatch.setattr(Sieve, "solve_many", solve_many)
    _no_solve(monkeypatch)
    frontend.configure(fallback=lambda *a: "z3", rows=256, certify=True)
    assert frontend.prefetch([cs]) == 1
    key = tuple(t.node for t in cs)
    assert key in frontend.sieve().witnesses
    rejected, hits = SolverStatistics().sieve_rejected, SolverStatistics().sieve_hits
    assert frontend.get_model(cs) == "z3"
    assert SolverStatistics().sieve_rejected == rejected + 1
    assert SolverStatistics().sieve_hits == hits
    assert key not in frontend.sieve().witnesses  # not left to seed the query's children
    # without certification the same parked witness is the model
    frontend.configure(certify=False)
    assert frontend.prefetch([cs]) == 1
    m = frontend.get_model(cs)
    assert isinstance(m, Model) and m.values["i"] == 9


def test_configure_reset_and_forget_witnesses_clear_the_table(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    cs = tuple(dict(qs)["selector"])
    frontend.configure(fallback=lambda *a: "fallback", **KW)
    for clear in (lambda: frontend.configure(enabled=True), frontend.forget_witnesses,
                  frontend.reset):
        assert frontend.prefetch([cs]) == 1 and len(frontend._parked()) == 1
        clear()
        assert len(frontend._parked()) == 0
        if clear is frontend.reset:
            frontend.configure(fallback=lambda *a: "fallback", **KW)
    # the table is bounded, oldest dropped
    monkeypatch.setattr(frontend, "PARKED_MAX", 2)
    css = [tuple(dict(qs)[n]) for n in ("selector", "owner_check", "balance")]
    assert frontend.prefetch(css) == 3
    keys = [tuple(t.node for t in c) for c in css]
    assert list(frontend._parked()) == keys[1:]


def test_objectives_and_a_disabled_sieve_are_untouched(monkeypatch):
    fake_batch.install(monkeypatch)
    ctx, qs = queries()
    cs = tuple(dict(qs)["selector"])
    seen = []
    frontend.configure(fallback=lambda c, mn, mx, enf: seen.append((mn, mx)) or "opt", **KW)
    assert frontend.prefetch([cs]) == 1
    x = BVS("objective", 256)
    assert frontend.get_model(cs, minimize=(x,)) == "opt" and seen == [((x,), ())]
    assert len(frontend._parked()) == 1  # the objective query never looked
    frontend.configure(enabled=False)
    assert frontend.prefetch([cs]) == 0


def test_prefetch_never_raises(monkeypatch):
    ctx, qs = queries()
    cs = tuple(dict(qs)["selector"])
    frontend.configure(fallback=lambda *a: "fallback", device=999)  # no such device
    assert frontend.prefetch([cs]) == 0
    assert frontend.prefetch(object()) == 0  # not even iterable
    frontend.reset()
    fake_batch.install(monkeypatch)
    frontend.configure(fallback=lambda *a: "fallback", **KW)

    def broken(self, *a, **kw):
        raise RuntimeError("device lost")

    monkeypatch.setattr(Sieve, "solve_many", broken)
    assert frontend.prefetch([cs]) == 0 and len(frontend._parked()) == 0
    assert frontend.prefetch([(object(),)]) == 0  # a constraint nothing can import
    assert isinstance(frontend.get_model(cs), Model)  # the ordinary path still answers
    with pytest.raises(UnsatError):
        frontend.get_model((False,))


class _VM:
    """A stand-in for LaserEVM: hook registration and open_states."""

    def __init__(self, states):
        self.open_states = states
        self.hooks = {}

    def register_laser_hooks(self, hook_type, hook):
        self.hooks.setdefault(hook_type, []).append(hook)


def test_plugin_hook_prefetches_the_open_states(monkeypatch):
    vm = _VM([types.SimpleNamespace(constraints=["a", "b"]),
              types.SimpleNamespace(constraints=["c"])])
    plugin.SievePlugin(modules=[]).initialize(vm)
    assert sorted(vm.hooks) == ["start_sym_exec", "stop_sym_exec"]  # off by default
    got = []
    monkeypatch.setattr(frontend, "prefetch", lambda qs: got.append(list(qs)) or len(got[-1]))
    vm = _VM(vm.open_states)
    plugin.SievePlugin(modules=[], prefetch=True).initialize(vm)
    (hook,) = vm.hooks["stop_sym_trans"]
    assert hook() == 2 and got == [[("a", "b"), ("c",)]]
    vm.open_states = []  # the states of the moment the hook runs, not of registration
    assert hook() == 0 and got[-1] == []
    monkeypatch.setenv("SIEVE_PREFETCH", "1")
    vm = _VM([])
    plugin.SievePlugin(modules=[]).initialize(vm)
    assert "stop_sym_trans" in vm.hooks
    monkeypatch.setenv("SIEVE_PREFETCH", "0")
    assert plugin.SievePlugin(modules=[]).prefetch is False
    assert plugin.SievePlugin(modules=[], prefetch=True).prefetch is True
