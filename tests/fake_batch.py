"""The batched round over the CPU stand-in of the device (tests/fake_device.py, which this module
leaves as it is): native.query_round_many as the loop over fake_query_round, which is its
contract -- every job's results equal mh_query_round's with the same arguments.  ROUNDS records
the job counts of the batches, so tests can see which queries shared a submission."""
from mythril_amd import native
from tests import fake_device

ROUNDS = []


def fake_query_round_many(ctx, jobs):
    ROUNDS.append(len(jobs))
    out = []
    for j in jobs:
        out.append(fake_device.fake_query_round(
            ctx, j["tapes"], j["assign"], j["guide"], j["seed"], j["global_base"], j["count"],
            j["n_cols"], tape_first=j.get("tape_first", 0), tape_count=j.get("tape_count"),
            mode=j.get("mode", native.MODE_FIRST_HIT)))
    return out


def install(monkeypatch):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(native, "query_round_many", fake_query_round_many)
    del ROUNDS[:]
