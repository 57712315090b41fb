"""Sieve(spares=K, batch_spares=True) on an MI355X: the JUMPI lists of tests/spares_cases.py
through solve_many give what the same call gives on the CPU stand-in (tests/fake_hits_many.py) and
what solve() gives on the list in order on the device -- witnesses, indices, spares, counters and
both stores; and through the front end a prefetch of a JUMPI's two successors parks two sieve
models answered by their parent's rows."""
import pytest

from mythril_amd import frontend
from mythril_amd.model import Model
from tests import fake_hits_many, spares_cases as SC
from tests.test_reference_fixtures import holds_original
from tests.test_solve_many_spares import _jumpi, batched, sequential

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_batched_spares_on_the_device(gpu_ctx, name):
    bs, qs = _jumpi(name)
    on_device = batched(bs, qs, batch_spares=True)
    recs, state, extra = on_device
    assert extra["batched_rounds"] >= 2 and extra["spare_hits"] >= 2
    assert "batch_refused" not in extra
    assert all(w is not None for w, _, _ in recs)
    # ... equals solve() in list order on the device
    want, want_state, _ = sequential(bs, qs)
    assert recs == want and state == want_state
    # ... and the same call on the stand-in
    mp = pytest.MonkeyPatch()
    try:
        fake_hits_many.install(mp)
        on_cpu = batched(bs, qs, batch_spares=True)
    finally:
        mp.undo()
    assert on_device[:2] == on_cpu[:2]
    for k in ("batched_rounds", "batches", "spare_rows", "spare_hits"):
        assert extra.get(k) == on_cpu[2].get(k), k


def test_prefetch_of_both_siblings_through_the_front_end(gpu_ctx):
    frontend.reset()
    try:
        calls = []
        frontend.configure(fallback=lambda c, *a: calls.append(c) or "fallback",
                           sieve_kwargs={"spares": 8, "batch_spares": True})
        ctx, parent, children = SC.one_group()
        s = frontend.sieve()
        assert s.spares == 8 and s.batch_spares
        assert isinstance(frontend.get_model(tuple(parent)), Model)
        siblings = [tuple(parent + [c]) for c in children]
        assert frontend.prefetch(siblings) == 2
        assert s.stats.extra.get("batched_rounds") == 2 and s.stats.extra.get("spare_hits") == 2
        rounds = s.stats.rounds
        for cs in siblings:
            m = frontend.get_model(cs)
            assert isinstance(m, Model) and holds_original(ctx, list(cs), m.schema, m.values)
        assert not calls and s.stats.rounds == rounds
    finally:
        frontend.reset()
