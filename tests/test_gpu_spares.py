"""The spare-witness policy (Sieve(spares=K); DESIGN §6 "Spare witnesses") on the device: the cases
of tests/test_spares.py give, with the same seed, the witnesses, indices, spare hits and rounds the
CPU stand-in gives; and a JUMPI's two siblings through frontend.get_model are both answered by the
sieve."""
import pytest

from mythril_amd import frontend
from mythril_amd.model import Model
from mythril_amd.sieve import Sieve
from tests import fake_hits, spares_cases as SC
from tests.test_reference_fixtures import holds_original
from tests.test_spares import check_policy

pytestmark = pytest.mark.gpu


def _sieve(spares):
    return Sieve(rows=256, budget_s=60.0, seed=SC.SEED, spares=spares)


@pytest.mark.parametrize("order", ["laser", "jumpi"])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_policy_on_the_device_equals_the_stand_in(gpu_ctx, name, order):
    on_device = check_policy(_sieve, name, order)
    mp = pytest.MonkeyPatch()
    try:
        fake_hits.install(mp)
        on_cpu = check_policy(_sieve, name, order)
    finally:
        mp.undo()
    assert on_device == on_cpu


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_spares_off_on_the_device_equals_the_stand_in(gpu_ctx, name):
    ctx, parent, children = SC.CASES[name]()
    qs = SC.sequence(parent, children, "jumpi")
    s = _sieve(0)
    try:
        on_device = SC.summary(SC.run(s, ctx, qs))
        assert not s.spare_witnesses and "spare_rows" not in s.stats.extra
    finally:
        s.close()
    mp = pytest.MonkeyPatch()
    try:
        fake_hits.install(mp)
        on_cpu = SC.summary(SC.run(_sieve(0), ctx, qs))
    finally:
        mp.undo()
    assert on_device == on_cpu


def test_both_siblings_through_get_model(gpu_ctx):
    """A JUMPI's two successors after their parent: both answered by the sieve from the
    parent's rows, the fallback never asked."""
    frontend.reset()
    try:
        calls = []
        frontend.configure(fallback=lambda c, *a: calls.append(c) or "fallback",
                           sieve_kwargs={"spares": 8})
        ctx, parent, children = SC.one_group()
        s = frontend.sieve()
        assert s.spares == 8
        assert isinstance(frontend.get_model(tuple(parent)), Model)
        rounds = s.stats.rounds
        for c in children:
            cs = parent + [c]
            m = frontend.get_model(tuple(cs))
            assert isinstance(m, Model) and holds_original(ctx, cs, m.schema, m.values)
        assert not calls
        assert s.stats.rounds == rounds + 2 and s.stats.extra.get("spare_hits") == 2
    finally:
        frontend.reset()
