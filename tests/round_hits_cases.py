"""Jobs for the batched listing round's parity check (mh_query_round_hits_many against
mh_query_round_hits, job by job): what tests/test_gpu_round_hits_many.py runs in the default library
and tests/noasm_round_hits_many_check.py in the C++ step() library.

The 17 jobs of tests/batch_cases.py (counts 1 / 63 / 64 / 65 / 4096; 1, 5 and 40 columns; a
70-tape set over two LDS chunks; streamed tapes; three register classes; keccak and EVM classes; a
tape sub-range; a job with no hit; one whose only generated hit is in the last partial wave; a
global_base above 2^32; all three generator forms) plus one over tests/hits_cases.py's set with
its spilling tape, each as a listing job with k from {1, 3, 64}, a third of them with spares
(n_rows 1, 5 and count; column subsets with the first and the last column).  coverage() reads off
the outputs that the batch held a tape with no hit, one with 1..k-1 hits, one with more than 64
and a job whose first hit is a scattered spare row.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from mythril_amd import native
from tests import batch_cases, hits_cases

KS = (1, 3, 64)
SPILL_JOB = "hits_spill"
SPARE_HIT_ROW = 2  # of conj_last_only's five spare rows, the one that satisfies its tape


def _limbs(v: int) -> List[int]:
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _random_rows(seed: int, n_rows: int, n_cols: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 1 << 32, size=(n_rows, n_cols, 8),
                                               dtype=np.uint64).astype(np.uint32)


def _spares(name: str, count: int):
    """(cols, values) of the jobs that carry spares, None for the others."""
    if name == "one_4096":  # one row; x0 = 0 satisfies x0 < 2^255: the first hit is row 0
        return [0], np.zeros((1, 1, 8), dtype=np.uint32)
    if name == "conj_last_only":
        # five rows over the first and the last of the five columns (and x3): row SPARE_HIT_ROW
        # alone holds the value the tape asks of x0, with x3 + x4 not overflowing 64 bits
        vals = _random_rows(51, 5, 3)
        vals[:, :, 2:] = 0  # (no x0 equals the value by chance; x3, x4 below 2^64)
        vals[SPARE_HIT_ROW, 0] = _limbs(batch_cases.last_only_value())
        vals[SPARE_HIT_ROW, 1:] = 0
        return [0, 3, 4], vals
    if name == "tree_63":  # as many rows as the round has: every row is a spare's
        return [0, 2], _random_rows(52, count, 2)
    if name == "kec_64":
        return [0, 17, 39], _random_rows(53, 5, 3)
    if name == "evm_65":
        return [39], _random_rows(54, count, 1)
    if name == SPILL_JOB:
        return [1], _random_rows(55, 1, 1)
    return None


def build(ctx) -> List[Dict]:
    """The 18 listing jobs, each with a buffer of its own (query_round_hits_many's job dicts
    plus "name")."""
    jobs = batch_cases.build(ctx)
    ts = hits_cases.build()[0]
    ct = ctx.compile(ts)
    first = hits_cases.SPILL_TAPE - 5  # six tapes, the spilling one last
    jobs.append(dict(name=SPILL_JOB, tapes=ct, assign=ctx.assignments(ts.n_vars, 130),
                     guide=batch_cases.HostGuide(batch_cases.flat_guide(ts.n_vars)),
                     seed=batch_cases.SEED + 99, global_base=14 << 24, count=130,
                     n_cols=ts.n_vars, tape_first=first, tape_count=6))
    for i, j in enumerate(jobs):  # (a listing job has no "mode": the key is left for coverage())
        j["k"] = KS[i % 3]
        j["spares"] = _spares(j["name"], j["count"])
    by = {j["name"]: j for j in jobs}
    by["conj_last_only"]["k"] = 3   # two hits: fewer than k
    by["one_4096"]["k"] = 64        # about half of 4096 rows hit: more than k
    by["conj_no_hit"]["k"] = 64
    return jobs


def _args(j: Dict):
    kw = {k: j[k] for k in ("tape_first", "tape_count") if k in j}
    return (j["tapes"], j["assign"], j["guide"], j["seed"], j["global_base"], j["count"],
            j["n_cols"], j["k"]), dict(kw, spares=j.get("spares"))


def run_sequential(ctx, jobs: List[Dict]):
    """Per job: query_round_hits' four results and a download of the buffer's rows [0, count)."""
    out = []
    for j in jobs:
        a, kw = _args(j)
        res = native.query_round_hits(ctx, *a, **kw)
        out.append(tuple(x.copy() for x in res) + (j["assign"].download(0, j["count"]),))
    return out


def run_batched(ctx, jobs: List[Dict]):
    """The same from one query_round_hits_many, over buffers overwritten first."""
    for j in jobs:
        j["assign"].generate(0xDEAD, 99)
    res = native.query_round_hits_many(ctx, jobs)
    return [tuple(x.copy() for x in r) + (j["assign"].download(0, j["count"]),)
            for r, j in zip(res, jobs)]


FIELDS = ("hits", "n_hits", "hit_count", "rows", "buffer contents")


def assert_equal(jobs: List[Dict], want, got) -> None:
    """Equal arrays per job, dtype and shape included."""
    for j, w, g in zip(jobs, want, got):
        for f, x, y in zip(FIELDS, w, g):
            assert x.dtype == y.dtype and x.shape == y.shape, (j["name"], f, x.shape, y.shape)
            assert np.array_equal(x, y), (j["name"], f)


def coverage(jobs: List[Dict], out) -> None:
    """The batch held what the module's docstring says (read off the outputs)."""
    by = {j["name"]: (j, o) for j, o in zip(jobs, out)}
    assert {j["k"] for j in jobs} == set(KS)
    assert sum(j["spares"] is not None for j in jobs) == 6
    assert any(j["spares"] is not None and len(j["spares"][1]) == j["count"] for j in jobs)
    # a tape with no hit
    j, (hits, nh, hc, rows, _) = by["conj_no_hit"]
    assert nh.tolist() == [0] and hc.tolist() == [0] and np.all(hits == native.NO_HIT)
    assert not rows.any()
    # one with 1..k-1 hits, whose first is a scattered spare row: the spare row that satisfies the
    # tape, then the generated row 64 of the last partial wave
    j, (hits, nh, hc, rows, _) = by["conj_last_only"]
    base = j["global_base"]
    assert 1 <= int(nh[0]) < j["k"] and hc.tolist() == [2]
    assert hits[0].tolist() == [base + SPARE_HIT_ROW, base + batch_cases.LAST_ONLY_COUNT - 1,
                                native.NO_HIT]
    cols, vals = j["spares"]
    assert len(vals) == 5 and cols[0] == 0 and cols[-1] == j["n_cols"] - 1
    assert np.array_equal(rows[0, 0][cols], vals[SPARE_HIT_ROW])
    # one with more than 64 hits: the list is full, ascending, and starts at the spare row
    j, (hits, nh, hc, rows, _) = by["one_4096"]
    assert int(hc[0]) > 64 and int(nh[0]) == 64 == j["k"]
    assert hits[0, 0] == j["global_base"] and np.all(np.diff(hits[0].astype(np.int64)) > 0)
    # the spilling tape ran
    j, _ = by[SPILL_JOB]
    assert j["tape_first"] + j["tape_count"] == hits_cases.SPILL_TAPE + 1
    assert j["tapes"].spills()[hits_cases.SPILL_TAPE] > 0


def check(ctx) -> str:
    """The whole parity check on `ctx`; returns a one-line summary."""
    jobs = build(ctx)
    try:
        want = run_sequential(ctx, jobs)
        coverage(jobs, want)
        got = run_batched(ctx, jobs)
        assert_equal(jobs, want, got)
        listed = sum(int(o[1].sum()) for o in got)
        return "round_hits_many ok: %d jobs equal mh_query_round_hits, %d hits listed" % (
            len(jobs), listed)
    finally:
        close(jobs)


def close(jobs: List[Dict]) -> None:
    for j in jobs:
        j["assign"].close()
    for ct in {id(j["tapes"]): j["tapes"] for j in jobs}.values():
        ct.close()
