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


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    fake = "--fake" in sys.argv
    if fake:
        import pytest

        from tests import fake_hits

        fake_hits.install(pytest.MonkeyPatch())
        SIEVE_KW.update(rows=256, budget_s=60.0)
    path = argv[0] if argv else None
    k = int(argv[1]) if len(argv) > 1 else 16
    reps = int(argv[2]) if len(argv) > 2 else 5
    warmup = int(argv[3]) if len(argv) > 3 else 3
    n_paths = int(argv[4]) if len(argv) > 4 else 20
    path_len = int(argv[5]) if len(argv) > 5 else 16
    os.environ.pop("SIEVE_SPARES", None)  # the settings compared are this script's
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
