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

``--many N`` compares, on the same witnesses, sequential ``certify`` with one
``Certifier.certify_many`` over N of them (certify.py "resident, batched certification"), on the
LASER-shaped queries' prefixes and the planted LASER paths: ms per certified hit, the two paths
interleaved in every repetition, the batched one with a fresh Certifier (``many_cold``: batching
alone, every chunk compiled) and with its chunks kept (``many_resident``).  ``--resident``
compares them query by query on the grown path's last 8 queries, the Certifier having seen the
path's earlier queries as under LASER.  No stage wrappers are installed in these modes.

    python scripts/certify_cost.py --many 64
    python scripts/certify_cost.py --resident [path_shape] [path_length]
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


def hits_of(s, ctx, nodes, first=1):
    """(model, constraints) of every prefix of `nodes` the sieve answers, in LASER order."""
    out = []
    for k in range(1, len(nodes) + 1):
        w = s.solve(ctx.b, nodes[:k], key=tuple(nodes[:k]))
        if w is not None and k >= first:
            out.append((Model(s, ctx, w.schema, w.values, w.index), nodes[:k]))
    return out


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3),
                max=round(max(xs), 3))


def compare_many(s, pool, n, workload, reps=7):
    """ms per certified hit over `n` witnesses of `pool` (cycled when it holds fewer)."""
    group = [pool[i % len(pool)] for i in range(n)]
    models, terms = [m for m, _ in group], [t for _, t in group]
    seq, cold, res = [], [], []
    resident = C.Certifier(s)
    resident.certify_many(models, terms)
    for _ in range(reps):
        gc.collect()
        t0 = time.perf_counter()
        want = [C.certify(m, t) for m, t in group]
        seq.append((time.perf_counter() - t0) * 1e3 / n)
        fresh = C.Certifier(s)
        t0 = time.perf_counter()
        got = fresh.certify_many(models, terms)
        cold.append((time.perf_counter() - t0) * 1e3 / n)
        fresh.close()
        t0 = time.perf_counter()
        again = resident.certify_many(models, terms)
        res.append((time.perf_counter() - t0) * 1e3 / n)
        assert [bool(v) for v in want] == [bool(v) for v in got] == [bool(v) for v in again]
    resident.close()
    print(json.dumps(dict(workload=workload, many=n, witnesses=len(pool), reps=reps,
                          unit="ms per certified hit", sequential=spread(seq),
                          many_cold=spread(cold), many_resident=spread(res),
                          constraints_median=statistics.median(len(t) for t in terms))),
          flush=True)


def main_many(n):
    s = Sieve()
    ctx, qs = queries()
    pool = []
    for name, _ in qs:
        if not name.startswith("unsat"):
            pool += hits_of(s, ctx, [c.node for c in dict(qs)[name]])
    compare_many(s, pool, n, "laser-shaped queries, every prefix hit")
    pool = []
    for seed in range(10):
        ctx, cs, _, _ = planted_path("laser", seed, 16)
        pool += hits_of(s, ctx, [c.node for c in cs], first=3)
    compare_many(s, pool, n, "planted LASER paths 10 x 16, prefixes >= 3")
    s.close()


def main_resident(shape, length, reps=5):
    s = Sieve()
    ctx, cs = grow(shape, length)
    nodes = [c.node for c in cs]
    # the hits among the last 9 prefixes: the first is the parent LASER leaves certified behind
    # it, the others are measured
    tail = hits_of(s, ctx, nodes, first=len(nodes) - 8)
    prime, last = tail[:1], tail[1:]
    resident = C.Certifier(s)
    t0 = time.perf_counter()
    for m, t in prime:
        resident.certify(m, t)
    prime_ms = (time.perf_counter() - t0) * 1e3
    per_query = []
    for m, t in last:
        seq, res = [], []
        compiles = resident.stats["chunk_compiles"]
        for r in range(reps):
            gc.collect()
            t0 = time.perf_counter()
            want = C.certify(m, t)
            seq.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            got = resident.certify(m, t)
            res.append((time.perf_counter() - t0) * 1e3)
            assert bool(want) == bool(got)
        # the first resident run is the LASER child's: it compiles the new chunk (at most one)
        per_query.append(dict(constraints=len(t), sequential=spread(seq),
                              resident_first=round(res[0], 3), resident_again=spread(res[1:]),
                              chunks_compiled=resident.stats["chunk_compiles"] - compiles))
    print(json.dumps(dict(workload="%s-%d in LASER order, last %d hits" % (shape, length, len(last)),
                          unit="ms per certification", prime_parent_ms=round(prime_ms, 3),
                          sequential_median=round(statistics.median(
                              q["sequential"]["median"] for q in per_query), 3),
                          resident_first_median=round(statistics.median(
                              q["resident_first"] for q in per_query), 3),
                          resident_again_median=round(statistics.median(
                              q["resident_again"]["median"] for q in per_query), 3),
                          queries=per_query)), flush=True)
    resident.close()
    s.close()


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--many" in sys.argv:
        return main_many(int(sys.argv[sys.argv.index("--many") + 1]))
    shape = argv[0] if argv else "ether_thief"
    length = int(argv[1]) if len(argv) > 1 else 400
    if "--resident" in sys.argv:
        return main_resident(shape, length)
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
