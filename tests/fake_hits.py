"""The CPU stand-in's hit listing (test infrastructure only): native.run_hits, Assignments.scatter
and native.query_round_hits restated on tests/fake_device.py's buffer and oracle evaluation, through
tests/hits_ref.py.  ``install(monkeypatch)`` installs fake_device's stand-ins and these."""
from mythril_amd import native
from oracle import smt_eval as E

from . import fake_device, hits_ref


class HitsAssign(fake_device.FakeAssign):
    def scatter(self, first, cols, values):
        cols = [int(c) for c in cols]
        assert all(a < b for a, b in zip(cols, cols[1:])) and all(c < self.n_vars for c in cols)
        assert first + len(values) <= self.capacity
        if not cols:
            return
        for r in range(len(values)):  # (a generated row holds the guide's columns only)
            row = list(self.rows[first + r])
            self.rows[first + r] = row + [0] * (cols[-1] + 1 - len(row))
        hits_ref.scatter(self.rows, first, cols, values)


class HitsContext(fake_device.FakeContext):
    def assignments(self, n_vars, capacity):
        return HitsAssign(n_vars, capacity)


def fake_run_hits(ctx, tapes, assign, k, n_cols, *, tape_first=0, tape_count=None, row_first=0,
                  row_count=None, index_base=0):
    tc = tapes.n_tapes - tape_first if tape_count is None else tape_count
    rc = assign.capacity - row_first if row_count is None else row_count
    assert 1 <= k <= native.HITS_MAX and 1 <= rc <= native.HITS_MAX_ROWS
    bools = [[bool(E.evaluate(tapes.tapes[tape_first + t], tapes.pool, assign.rows[r]))
              for r in range(row_first, row_first + rc)] for t in range(tc)]
    table = {r: list(assign.rows[r]) + [0] * (n_cols - len(assign.rows[r]))
             for r in range(row_first, row_first + rc)}
    return hits_ref.run_hits(bools, table, row_first, index_base, k, n_cols)


def fake_query_round_hits(ctx, tapes, assign, guide, seed, global_base, count, n_cols, k, *,
                          spares=None, tape_first=0, tape_count=None):
    assign.generate_guided(seed, guide.arrays(), global_base=global_base, count=count)
    if spares is not None:
        cols, values = spares
        assert len(values) <= count
        assign.scatter(0, cols, values)
    return fake_run_hits(ctx, tapes, assign, k, n_cols, tape_first=tape_first,
                         tape_count=tape_count, row_count=count, index_base=global_base)


def install(monkeypatch):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(native, "Context", HitsContext)
    monkeypatch.setattr(native, "run_hits", fake_run_hits)
    monkeypatch.setattr(native, "query_round_hits", fake_query_round_hits)
