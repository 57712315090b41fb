#!/usr/bin/env python3
"""What spare witnesses (Sieve(spares=K); DESIGN §6 "Spare witnesses") cost and answer, on an
MI355X in one session, SIEVE_SPARES at 0 against K (default 16) on Sieves made alike:

* the LASER-shaped queries of tests/laser_like.py (the SAT shapes and the UNSAT hard variants, the
  ones scripts/sieve_queries.py times), each path asked in three orders: ``laser`` (every prefix,
  its parent first), ``jumpi`` (at every constraint both successors, svm.py:243-262) and ``bfs``
  (tests/bfs_order.py: the open states of a level ask both branches back to back);
* the planted random family of scripts/planted_recall.py (SAT by construction, LASER order).

Per workload and setting: the queries, the share answered by an ancestor's rows (``spare_hits``),
recall (answered / asked; on the planted family every query is SAT), hit and miss latency p50 / p99;
then the first round's device time (mh_ctx_kernel_time) and wall time on one staged query,
``query_round`` against ``query_round_hits``.  `warmup` runs are dropped, then `reps` are kept:
every figure is the median over the kept runs with their min and max.

    python scripts/spares_cost.py [out.jsonl] [K=16] [reps=5] [warmup=3] [n_paths=20] [path_len=16]
                                  [--fake]

One JSON line per (workload, order, setting), appended to out.jsonl when given.  --fake runs the
policy on the CPU stand-in (tests/fake_hits.py; small rounds, no device times): a dry run.

--batched measures spares in batched first rounds instead (Sieve(batch_spares=True)):
the same two families in ``jumpi`` and ``bfs`` order through Sieve.solve_many, 8 and 64 queries
per list, under three settings -- SIEVE_SPARES=0 (the baseline), K without batch_spares, K with it
-- reporting per query the total / host / round milliseconds, recall, the spare-hit share and the
queries asked; then the primitive: device and wall milliseconds of ``query_round_hits_many`` at k =
K against ``query_round_many`` and against ``query_round_hits`` one by one, on the same 8 and 64
jobs of 4096 rows.
"""
import gc
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))

import numpy as np  # noqa: E402

from mythril_amd import native  # noqa: E402
from mythril_amd.sieve import Sieve  # noqa: E402
from mythril_amd.smt import Not  # noqa: E402
from tests.bfs_order import bfs_queries  # noqa: E402
from tests.laser_like import hard_queries, queries  # noqa: E402
from tests.planted import planted_path  # noqa: E402


SIEVE_KW = {}  # --fake: the stand-in's small rounds


def _mmm(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)} if v else None


def _pcts(ms):
    if not ms:
        return None
    a = np.array(ms)
    return float(np.percentile(a, 50)), float(np.percentile(a, 99))


def ordered(cs, order, ask):
    """Ask the path's queries in `order`; ask(constraints) -> answered?"""
    if order == "laser":
        for k in range(1, len(cs) + 1):
            ask(cs[:k])
    elif order == "jumpi":
        for k in range(len(cs)):
            ask(cs[:k] + [cs[k]])
            ask(cs[:k] + [Not(cs[k])])
    else:
        by_node = {}
        for c in cs:
            by_node[c.node] = c
            n = Not(c)
            by_node[n.node] = n
        dropped = set()
        nodes = [c.node for c in cs]
        negs = [Not(c).node for c in cs]
        for q in bfs_queries(nodes, negs, 1, 4, seed=1, dropped=dropped):
            if not ask([by_node[n] for n in q]):
                dropped.add(tuple(q))


def laser_paths():
    for kind, build in (("sat", queries), ("unsat", hard_queries)):
        for name, _ in build()[1]:
            ctx, qs = build()  # fresh terms: nothing memoised on the nodes
            yield ctx, dict(qs)[name]


def run_once(spares, workload, order, n_paths, path_len):
    """One pass of a workload on a fresh Sieve: (queries, answered, spare hits, hit ms, miss ms)."""
    s = Sieve(spares=spares, **SIEVE_KW)
    hit_ms, miss_ms = [], []
    n = [0, 0]

    def asker(ctx):
        def ask(cs):
            nodes = [c.node for c in cs]
            gc.collect()
            t0 = time.perf_counter()
            try:
                w = s.solve(ctx.b, nodes, key=tuple(nodes))
            except Exception:  # noqa: BLE001 - the front end falls back on any error
                w = None
            dt = (time.perf_counter() - t0) * 1e3
            n[0] += 1
            n[1] += w is not None
            (hit_ms if w is not None else miss_ms).append(dt)
            return w is not None
        return ask

    try:
        if workload == "laser_like":
            for ctx, cs in laser_paths():
                if hasattr(s.ctx, "clear_cache"):
                    s.ctx.clear_cache()
                ordered(cs, order, asker(ctx))
        else:
            for seed in range(n_paths):
                ctx, cs, _, _ = planted_path("random", seed, path_len)
                ordered(cs, order, asker(ctx))
        return n[0], n[1], s.stats.extra.get("spare_hits", 0), hit_ms, miss_ms
    finally:
        s.close()


def measure(spares, workload, order, reps, warmup, n_paths, path_len):
    runs = [run_once(spares, workload, order, n_paths, path_len)
            for _ in range(warmup + reps)][warmup:]
    q, answered, sp_hits = runs[0][0], runs[0][1], runs[0][2]
    hp = [_pcts(r[3]) for r in runs if r[3]]
    mp = [_pcts(r[4]) for r in runs if r[4]]
    return {"workload": workload, "order": order, "spares": spares, "reps": reps,
            "warmup": warmup, "queries": q, "answered": answered,
            "recall": round(answered / max(q, 1), 4),
            "spare_hits": sp_hits, "spare_hit_share": round(sp_hits / max(q, 1), 4),
            "same_counts_every_run": all(r[:3] == runs[0][:3] for r in runs),
            "hit_ms_p50": _mmm([p[0] for p in hp]), "hit_ms_p99": _mmm([p[1] for p in hp]),
            "miss_ms_p50": _mmm([p[0] for p in mp]), "miss_ms_p99": _mmm([p[1] for p in mp])}


def first_round(k, reps, warmup):
    """The first round of one staged query (ether_thief's whole path), run by both entry points on
    the same tapes, guide, seed and rows: the launches' device time and the call's wall time."""
    ctx, qs = queries()
    cs = dict(qs)["ether_thief"]
    s = Sieve()
    out = []
    try:
        st = s._stage(ctx.b, [c.node for c in cs], None, False, 1)
        columns = st.host.columns
        assign = s._buffer(len(columns))
        n = s.first_rows
        calls = {
            "query_round": lambda: native.query_round(
                s.ctx, st.ct, assign, st.guide, s.seed, 1 << 24, n, len(columns),
                mode=native.MODE_FIRST_HIT),
            "query_round_hits": lambda: native.query_round_hits(
                s.ctx, st.ct, assign, st.guide, s.seed, 1 << 24, n, len(columns), k)}
        s.ctx.enable_timing(True)
        for name, call in calls.items():
            dev, wall = [], []
            for i in range(warmup + reps):
                s.ctx.kernel_time()
                t0 = time.perf_counter()
                call()
                w = (time.perf_counter() - t0) * 1e3
                ms, spans = s.ctx.kernel_time()
                if i >= warmup:
                    dev.append(ms)
                    wall.append(w)
            out.append({"first_round": name, "k": k if name.endswith("hits") else None, "rows": n,
                        "groups": st.ct.n_tapes, "columns": len(columns), "reps": reps,
                        "warmup": warmup, "spans": spans, "device_ms": _mmm(dev),
                        "wall_ms": _mmm(wall)})
        s.ctx.enable_timing(False)
        st.close()
    finally:
        s.close()
    return out


def query_list(workload, order, n_paths, path_len):
    """The family's queries in `order`, path after path: [(builder, root nodes)].  (In bfs order
    no branch is dropped: the list does not depend on a setting's answers.)"""
    out = []

    def collect(ctx):
        def ask(cs):
            out.append((ctx.b, [c.node for c in cs]))
            return True
        return ask

    if workload == "laser_like":
        for ctx, cs in laser_paths():
            ordered(cs, order, collect(ctx))
    else:
        for seed in range(n_paths):
            ctx, cs, _, _ = planted_path("random", seed, path_len)
            ordered(cs, order, collect(ctx))
    return out


SETTINGS = (("spares0", 0, False), ("spares", None, False), ("batch_spares", None, True))


def run_many_once(qs, per, spares, batch_spares):
    """The list through solve_many, `per` queries a call, on a fresh Sieve: (queries, answered,
    spare hits, batched first rounds, total ms, host ms, round ms)."""
    s = Sieve(spares=spares, batch_spares=batch_spares, **SIEVE_KW)
    try:
        gc.collect()
        t0 = time.perf_counter()
        for lo in range(0, len(qs), per):
            part = qs[lo:lo + per]
            s.solve_many([b for b, _ in part], [r for _, r in part],
                         keys=[tuple(r) for _, r in part])
        total = (time.perf_counter() - t0) * 1e3
        st = s.stats
        return (st.queries, st.hits, st.extra.get("spare_hits", 0),
                st.extra.get("batched_rounds", 0), total, st.host_s * 1e3,
                st.stage_s.get("run", 0.0) * 1e3)
    finally:
        s.close()


def measure_many(k, workload, order, per, reps, warmup, n_paths, path_len):
    qs = query_list(workload, order, n_paths, path_len)
    recs = []
    for name, spares, batch_spares in SETTINGS:
        spares = k if spares is None else spares
        runs = [run_many_once(qs, per, spares, batch_spares)
                for _ in range(warmup + reps)][warmup:]
        q = max(runs[0][0], 1)
        recs.append({"batched": name, "workload": workload, "order": order, "per_list": per,
                     "spares": spares, "batch_spares": batch_spares, "reps": reps,
                     "warmup": warmup, "queries": runs[0][0], "answered": runs[0][1],
                     "recall": round(runs[0][1] / q, 4), "spare_hits": runs[0][2],
                     "spare_hit_share": round(runs[0][2] / q, 4), "batched_rounds": runs[0][3],
                     "same_counts_every_run": all(r[:4] == runs[0][:4] for r in runs),
                     "total_ms_per_query": _mmm([r[4] / q for r in runs]),
                     "host_ms_per_query": _mmm([r[5] / q for r in runs]),
                     "round_ms_per_query": _mmm([r[6] / q for r in runs])})
    return recs


def primitive(k, n_jobs, reps, warmup):
    """The same n_jobs first rounds of 4096 rows (ether_thief's whole path, a buffer per job) by
    query_round_many, by query_round_hits_many at k and by query_round_hits one by one."""
    ctx, qs = queries()
    cs = dict(qs)["ether_thief"]
    s = Sieve(first_rows=4096)
    bufs, out = [], []
    try:
        st = s._stage(ctx.b, [c.node for c in cs], None, False, 1)
        n_cols, n = len(st.host.columns), s.first_rows
        bufs = [s.ctx.assignments(s._col_capacity(n_cols), n) for _ in range(n_jobs)]
        jobs = [dict(tapes=st.ct, assign=a, guide=st.guide, seed=s.seed, global_base=(i + 1) << 24,
                     count=n, n_cols=n_cols, k=k, mode=native.MODE_FIRST_HIT)
                for i, a in enumerate(bufs)]
        calls = {
            "query_round_many": lambda: native.query_round_many(s.ctx, jobs),
            "query_round_hits_many": lambda: native.query_round_hits_many(s.ctx, jobs),
            "query_round_hits_each": lambda: [native.query_round_hits(
                s.ctx, st.ct, j["assign"], st.guide, s.seed, j["global_base"], n, n_cols, k)
                for j in jobs]}
        s.ctx.enable_timing(True)
        for name, call in calls.items():
            dev, wall = [], []
            for i in range(warmup + reps):
                s.ctx.kernel_time()
                t0 = time.perf_counter()
                call()
                w = (time.perf_counter() - t0) * 1e3
                ms, spans = s.ctx.kernel_time()
                if i >= warmup:
                    dev.append(ms)
                    wall.append(w)
            out.append({"primitive": name, "jobs": n_jobs, "k": None if name.endswith("_many")
                        and "hits" not in name else k, "rows": n, "groups": st.ct.n_tapes,
                        "columns": n_cols, "reps": reps, "warmup": warmup, "spans": spans,
                        "device_ms": _mmm(dev), "wall_ms": _mmm(wall),
                        "device_ms_per_job": _mmm([d / n_jobs for d in dev]),
                        "wall_ms_per_job": _mmm([w / n_jobs for w in wall])})
        s.ctx.enable_timing(False)
        st.close()
    finally:
        for a in bufs:
            a.close()
        s.close()
    return out


def main_batched(path, k, reps, warmup, n_paths, path_len, fake):
    recs = []
    for workload in ("laser_like", "planted_random"):
        for order in ("jumpi", "bfs"):
            for per in (8, 64):
                for r in measure_many(k, workload, order, per, reps, warmup, n_paths, path_len):
                    recs.append(r)
                    print(json.dumps(r), flush=True)
    for n_jobs in ([] if fake else (8, 64)):
        for r in primitive(k, n_jobs, max(reps, 20), warmup):
            recs.append(r)
            print(json.dumps(r), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    fake = "--fake" in sys.argv
    if fake:
        import pytest

        from tests import fake_hits_many

        fake_hits_many.install(pytest.MonkeyPatch())
        SIEVE_KW.update(rows=256, budget_s=60.0)
    path = argv[0] if argv else None
    k = int(argv[1]) if len(argv) > 1 else 16
    reps = int(argv[2]) if len(argv) > 2 else 5
    warmup = int(argv[3]) if len(argv) > 3 else 3
    n_paths = int(argv[4]) if len(argv) > 4 else 20
    path_len = int(argv[5]) if len(argv) > 5 else 16
    os.environ.pop("SIEVE_SPARES", None)  # the settings compared are this script's
    os.environ.pop("SIEVE_BATCH_SPARES", None)
    if "--batched" in sys.argv:
        return main_batched(path, k, reps, warmup, n_paths, path_len, fake)
    recs = []
    for workload, orders in (("laser_like", ("laser", "jumpi", "bfs")), ("planted_random",
                                                                         ("laser",))):
        for order in orders:
            for spares in (0, k):
                recs.append(measure(spares, workload, order, reps, warmup, n_paths, path_len))
                print(json.dumps(recs[-1]), flush=True)
    for r in ([] if fake else first_round(k, max(reps, 20), warmup)):
        recs.append(r)
        print(json.dumps(r), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
