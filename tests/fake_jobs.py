"""CPU stand-ins for the batched values calls of mythril_amd.native (mh_eval_values_jobs,
mh_tables_create_many), built on tests/fake_tables.py and tests/fake_device.py (test
infrastructure only).  ``install(monkeypatch)`` installs those modules' stand-ins and these.

A job is evaluated by the single call's stand-in it stands for, so what the certifier's batched
path computes here is by construction what its sequential path computes; the device test
(tests/test_gpu_values_jobs.py) pins the real entry point to the real single calls.
"""
from mythril_amd import native
from tests import fake_device, fake_tables

SUBMISSIONS = [0]   # eval_values_jobs submissions (ceil(jobs / VALUES_JOBS_MAX) per call)
CREATE_MANY = [0]   # tables_create_many calls


def fake_tables_create_many(ctx, sets):
    CREATE_MANY[0] += 1
    return [fake_tables.FakeTables(ctx, tabs) for tabs in sets]  # one invalid set raises: none


def fake_eval_values_jobs(ctx, jobs):
    out = []
    for tapes, tables, ids, assign, row in jobs:
        if row not in assign.rows:
            raise native.SieveError(native.MH_E_INVALID, "mh_eval_values_jobs: row out of bounds")
        if tables is None:
            out.append(fake_device.fake_eval_values_many(ctx, tapes, list(ids), assign, row))
            fake_device.LAUNCHES[0] -= 1  # (the single call's counter counts single calls)
        else:
            out.append(fake_tables.fake_eval_values_tables(ctx, tapes, tables, list(ids), assign,
                                                           row, 1)[:, :, 0])
    SUBMISSIONS[0] += -(-len(jobs) // native.VALUES_JOBS_MAX)
    return out


def install(monkeypatch):
    fake_tables.install(monkeypatch)
    monkeypatch.setattr(native, "tables_create_many", fake_tables_create_many)
    monkeypatch.setattr(native, "eval_values_jobs", fake_eval_values_jobs)
