#!/usr/bin/env python3
"""What certifying a hit costs (DESIGN §6 "Certification of a hit"), split by stage.

For each workload every query is solved as LASER issues it (each prefix of the path in order, with
its key) and every witness is certified (mythril_amd/certify.py); the certification's stages are
timed by wrapping them:

* ``table_build``  ExtModel.from_model (Model.tables' batch and, with a keccak inverse, the forward
                   applications' batch; their own compiles and launches are inside this figure)
* ``ext_lower``    the extensional lowering of the constraints (memoised per node)
* ``compile``      Sieve.compile of the constraints' tapes (a child finds its parent's in the
                   ctx's tape cache)
* ``table_upload`` native.tables_create (packing and mh_tables_create)
* ``launch``       native.eval_values_tables (launch, copy back, sync)

Workloads: the LASER-shaped SAT queries of tests/laser_like.py (what scripts/sieve_queries.py
runs), the final query cold (tape cache cleared, fresh terms) and as a LASER child; a path grown
to N constraints in LASER order (tests/laser_paths.grow: EtherThief-400 by default), the last 8
queries; planted LASER paths.  ``solve`` is the hit itself, so certification off is that column
alone.  One JSON line per workload, medians in milliseconds.

    python scripts/certify_cost.py [path_shape=ether_thief] [path_length=400]
"""
import gc
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from mythril_amd import certify as C  # noqa: E402
from mythril_amd import native  # noqa: E402
from mythril_amd.model import Model  # noqa: E402
from mythril_amd.sieve import Sieve  # noqa: E402
from tests.laser_like import queries  # noqa: E402
from tests.laser_paths import grow  # noqa: E402
from tests.planted import planted_path  # noqa: E402

T = {}
DEPTH = [0]  # compiles and launches inside table_build belong to it


def timed(name, fn, outer=False):
    def w(*a, **k):
        if DEPTH[0] and not outer:
            return fn(*a, **k)
        t0 = time.perf_counter()
        DEPTH[0] += outer
        try:
            return fn(*a, **k)
        finally:
            DEPTH[0] -= outer
            T[name] = T.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    return w


def install():
    C.ExtModel.from_model = classmethod(timed("table_build", C.ExtModel.from_model.__func__,
                                              outer=True))
    C.ext_lower = timed("ext_lower", C.ext_lower)
    Sieve.compile = timed("compile", Sieve.compile)
    native.tables_create = timed("table_upload", native.tables_create)
    native.eval_values_tables = timed("launch", native.eval_values_tables)


def solve_and_certify(s, ctx, nodes):
    """(stage times of this query or None for a miss)."""
    gc.collect()
    t0 = time.perf_counter()
    w = s.solve(ctx.b, nodes, key=tuple(nodes))
    dt = (time.perf_counter() - t0) * 1e3
    if w is None:
        return None
    T.clear()
    t0 = time.perf_counter()
    v = C.certify(Model(s, ctx, w.schema, w.values, w.index), nodes)
    rec = dict(T, solve=dt, certify=(time.perf_counter() - t0) * 1e3, ok=bool(v))
    return rec


def med(rows):
    keys = sorted({k for r in rows for k in r if k != "ok"})
    out = {k: round(statistics.median([r.get(k, 0.0) for r in rows]), 3) for k in keys}
    out["hits"] = len(rows)
    out["rejected"] = sum(1 for r in rows if not r["ok"])
    return out


def main():
    shape = sys.argv[1] if len(sys.argv) > 1 else "ether_thief"
    length = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    install()
    s = Sieve()
    ctx, qs = queries()
    solve_and_certify(s, ctx, [c.node for c in qs[0][1]])  # warm-up: runtime, code objects
    child, cold = [], []
    for name, _ in qs:
        if name.startswith("unsat"):
            continue
        s.ctx.clear_cache()
        ctx, fresh = queries()
        nodes = [c.node for c in dict(fresh)[name]]
        rec = None
        for k in range(1, len(nodes) + 1):
            rec = solve_and_certify(s, ctx, nodes[:k])
        if rec is not None:
            child.append(rec)
        s.ctx.clear_cache()
        ctx, fresh = queries()
        nodes = [c.node for c in dict(fresh)[name]]
        rec = solve_and_certify(s, ctx, nodes)
        if rec is not None:
            cold.append(rec)
    print(json.dumps(dict(med(child), workload="laser-shaped queries, as a LASER child")), flush=True)
    print(json.dumps(dict(med(cold), workload="laser-shaped queries, cold")), flush=True)
    s.ctx.clear_cache()
    ctx, cs = grow(shape, length)
    nodes = [c.node for c in cs]
    rows = [solve_and_certify(s, ctx, nodes[:k]) for k in range(1, len(nodes) + 1)]
    last = [r for r in rows[-8:] if r is not None]
    if last:
        print(json.dumps(dict(med(last), workload="%s-%d in LASER order, last 8" % (shape, length),
                              prefix_hits=sum(r is not None for r in rows))), flush=True)
    rows = []
    for seed in range(10):
        ctx, cs, _, _ = planted_path("laser", seed, 16)
        nodes = [c.node for c in cs]
        for k in range(1, len(nodes) + 1):
            r = solve_and_certify(s, ctx, nodes[:k])
            if r is not None and k >= 3:
                rows.append(r)
    print(json.dumps(dict(med(rows), workload="planted LASER paths 10 x 16, prefixes >= 3")),
          flush=True)
    s.close()


if __name__ == "__main__":
    main()
