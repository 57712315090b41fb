"""The batched listing round over the CPU stand-in of the device (test infrastructure only):
native.query_round_hits_many as tests/fake_hits.fake_query_round_hits applied per job, which is its
contract -- every job's results equal mh_query_round_hits' with the same arguments.  ROUNDS records
the job counts of the batches.  ``install(monkeypatch)`` installs tests/fake_batch.py's and
tests/fake_hits.py's stand-ins and this one."""
from mythril_amd import native
from tests import fake_batch, fake_hits

ROUNDS = []


def fake_query_round_hits_many(ctx, jobs):
    ROUNDS.append(len(jobs))
    return [fake_hits.fake_query_round_hits(
        ctx, j["tapes"], j["assign"], j["guide"], j["seed"], j["global_base"], j["count"],
        j["n_cols"], j["k"], spares=j.get("spares"), tape_first=j.get("tape_first", 0),
        tape_count=j.get("tape_count")) for j in jobs]


def install(monkeypatch):
    fake_batch.install(monkeypatch)  # (first: fake_hits' Context replaces fake_device's)
    fake_hits.install(monkeypatch)
    monkeypatch.setattr(native, "query_round_hits_many", fake_query_round_hits_many)
    del ROUNDS[:]
