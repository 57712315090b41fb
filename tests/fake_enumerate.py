"""A CPU stand-in for the enumerating generator (mh_assign_enumerate / mh_query_enumerate), beside
tests/fake_device.py (test infrastructure only: the product path never imports this).

``install(monkeypatch)`` installs fake_device's stand-ins and adds native.query_enumerate on
them: the rows come from mythril_amd.decide.enumerate_rows (the restatement
tests/test_gpu_enumerate.py pins against the kernel), the run is fake_device's.  The domains are
the library's own (mh_domains_build is host only)."""
from mythril_amd import decide, native

from tests import fake_device

WINDOWS = []  # (global_base, count) of every window enumerated, in order


def fake_enumerate(assign, domains, global_base=0, first=0, count=None):
    count = assign.capacity - first if count is None else count
    assert first + count <= assign.capacity
    assert all(c < assign.n_vars for c in domains.cols)
    for r, vals in enumerate(decide.enumerate_rows(domains, global_base, count)):
        row = list(assign.rows.get(first + r, ()))
        row += [0] * (assign.n_vars - len(row))  # columns outside the domains stay as they were
        for c, v in zip(domains.cols, vals):
            row[c] = v
        assign.rows[first + r] = row


def fake_query_enumerate(ctx, tapes, assign, domains, global_base, count, n_cols, *, tape=0,
                         mode=native.MODE_FIRST_HIT):
    WINDOWS.append((global_base, count))
    fake_enumerate(assign, domains, global_base, 0, count)
    return fake_device.fake_run_rows(ctx, tapes, assign, n_cols, tape_first=tape, tape_count=1,
                                     row_count=count, index_base=global_base, mode=mode)


def install(monkeypatch):
    fake_device.install(monkeypatch)
    del WINDOWS[:]
    monkeypatch.setattr(native, "query_enumerate", fake_query_enumerate)
    monkeypatch.setattr(fake_device.FakeAssign, "enumerate", fake_enumerate, raising=False)
