#!/usr/bin/env python3
"""What batching first rounds saves (DESIGN §6 "Batched rounds"): N independent feasibility
queries answered by Sieve.solve_many -- their first rounds in one device submission
(mh_query_round_many) -- against the same N answered by Sieve.solve one after another, on the same
commit, at N = 1, 2, 8, 32, 128.

Two workloads: the LASER-shaped queries of tests/laser_like.py (the 15 shapes, repeated on fresh
term contexts to reach N) and planted LASER paths (tests/planted.py: one 12-constraint path per
query, a seed each) -- N open world states asked at the start of a transaction round
(laser/ethereum/svm.py:201-203).  Per (workload, N, mode) one JSON line: milliseconds per query,
median of BATCH_REPS (default 9) repetitions, split into the host stage (native build, harvest,
compile: stats.host_s), the device rounds (the "run" stage: every round's submission and wait)
and the rest; hits; device submissions.  Every repetition builds its queries on fresh term
contexts and starts with the compiled-tape cache and the witness store empty, after a
gc.collect(), as scripts/sieve_queries.py does.

With --parent DIR (a built checkout of the parent commit) it then runs scripts/sieve_queries.py of
this tree and of DIR as child processes, two passes each, interleaved, and prints per pass the
median over the queries of ms_incremental and ms_cold: whether splitting Sieve._attempt into
stage + rounds slowed the sequential path, against the spread between the parent's own passes.
Each child runs under its own time limit; a child that fails ends the script.

    python scripts/batch_rounds.py [--parent DIR] [--sizes 1,2,8,32,128] [--out FILE]
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402


def laser_like_batch(n):
    """n LASER-shaped queries: the shapes of tests/laser_like.py in order, a fresh term context
    per pass over them."""
    from tests.laser_like import queries

    out = []
    while len(out) < n:
        ctx, qs = queries()
        for _, cs in qs:
            if len(out) < n:
                out.append((ctx.b, [c.node for c in cs]))
    return out


def planted_batch(n):
    from tests.planted import planted_path

    out = []
    for seed in range(n):
        ctx, cs, _, _ = planted_path("laser", seed, 12)
        out.append((ctx.b, [c.node for c in cs]))
    return out


WORKLOADS = {"laser_like": laser_like_batch, "planted_laser": planted_batch}


def one_rep(s, batch, many):
    """One timed repetition: (ms per query, host ms, run ms, hits, submissions per query)."""
    s.ctx.clear_cache()
    s.witnesses.clear()
    bs = [b for b, _ in batch]
    roots = [r for _, r in batch]
    keys = [tuple(r) for r in roots]
    st = s.stats
    host0, run0, rounds0 = st.host_s, st.stage_s.get("run", 0.0), st.rounds
    batches0, batched0 = st.extra.get("batches", 0), st.extra.get("batched_rounds", 0)
    gc.collect()
    t0 = time.perf_counter()
    if many:
        ws = s.solve_many(bs, roots, keys=keys, budget_s=60.0)
    else:
        ws = [s.solve(b, r, key=k, budget_s=60.0) for b, r, k in zip(bs, roots, keys)]
    total = time.perf_counter() - t0
    n = len(batch)
    # a batched first round is one submission for all of its queries
    subs = (st.rounds - rounds0) - (st.extra.get("batched_rounds", 0) - batched0) \
        + (st.extra.get("batches", 0) - batches0)
    return (1e3 * total / n, 1e3 * (st.host_s - host0) / n,
            1e3 * (st.stage_s.get("run", 0.0) - run0) / n, sum(w is not None for w in ws),
            subs / n)


def measure(sizes, reps, emit):
    from mythril_amd.sieve import Sieve
    from tests.laser_like import queries

    s = Sieve(budget_s=60.0)
    try:
        ctx, qs = queries()  # warm-up: the HIP runtime's lazy initialisation, the code objects
        s.solve(ctx.b, [c.node for c in qs[0][1]])
        s.solve_many(ctx.b, [[c.node for c in cs] for _, cs in qs[:4]])
        for name, make in WORKLOADS.items():
            for n in sizes:
                for many in (False, True):
                    got = [one_rep(s, make(n), many) for _ in range(reps)]
                    ms, host, run, hits, subs = (float(np.median([g[i] for g in got]))
                                                 for i in range(5))
                    emit(dict(workload=name, n=n, mode="solve_many" if many else "solve",
                              ms_per_query=round(ms, 4), host_ms=round(host, 4),
                              round_ms=round(run, 4), rest_ms=round(ms - host - run, 4),
                              hits=int(hits), submissions_per_query=round(subs, 3), reps=reps,
                              ms_all=[round(g[0], 4) for g in got]))
    finally:
        s.close()


def sequential_passes(parent, emit, limit_s):
    """scripts/sieve_queries.py of this tree and of `parent`, two passes each, interleaved."""
    for p in range(2):
        for label, root in (("this", HERE), ("parent", parent)):
            r = subprocess.run([sys.executable, os.path.join(root, "scripts", "sieve_queries.py")],
                               cwd=root, capture_output=True, text=True, timeout=limit_s)
            if r.returncode != 0:
                emit(dict(sequential=label, passno=p, error=r.stderr[-2000:], rc=r.returncode))
                return False
            recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            per = [x for x in recs if "query" in x and "ms_incremental" in x]
            emit(dict(sequential=label, passno=p, queries=len(per),
                      errors=sum("error" in x for x in recs),
                      ms_incremental_median=round(float(np.median(
                          [x["ms_incremental"] for x in per])), 4),
                      ms_cold_median=round(float(np.median([x["ms_cold"] for x in per])), 4),
                      ms_incremental_sum=round(sum(x["ms_incremental"] for x in per), 3),
                      host_stage_ms_sum=round(sum(
                          sum(v for k, v in x.get("stages_ms", {}).items()
                              if k in ("guide", "compile", "compile_wait")) for x in per), 3),
                      hits=sum(bool(x.get("hit")) for x in per)))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--sizes", default="1,2,8,32,128")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child-limit", type=float, default=240.0)
    a = ap.parse_args()
    reps = int(os.environ.get("BATCH_REPS", "9"))
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    measure([int(x) for x in a.sizes.split(",")], reps, emit)
    ok = True
    if a.parent:
        ok = sequential_passes(os.path.abspath(a.parent), emit, a.child_limit)
    if sink:
        sink.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
