#!/usr/bin/env python3
"""Device time of one repair iteration's steps (DESIGN §6 "repair"): mh_repair_score, _select and
_mutate on the chain queries of tests/repair_cases.py, at the policy's launch shape (K elites x
`per` children).  Times are the launches' own (mh_ctx_kernel_time: HIP events on the ctx stream),
medians over `reps`; the wall time of each call (its host side and the sync) beside them.

    python scripts/repair_cost.py [M=6,24,96] [K=64] [per=64] [reps=20]

One JSON line per M.
"""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from mythril_amd import native  # noqa: E402
from mythril_amd.sieve import LocalPool  # noqa: E402
from mythril_amd.tape import Tape, TapeSet  # noqa: E402
from tests.repair_cases import chain_query  # noqa: E402


def main():
    argv = sys.argv[1:]
    ms_ = [int(x) for x in argv[0].split(",")] if argv else [6, 24, 96]
    K = int(argv[1]) if len(argv) > 1 else 64
    per = int(argv[2]) if len(argv) > 2 else 64
    reps = int(argv[3]) if len(argv) > 3 else 20
    ctx = native.Context(0)
    rep = native.repair_open(ctx, 512, 1 << 16, 256)
    for m in ms_:
        tctx, cs = chain_query(m)
        cq = native.TermMirror.of(tctx.b).build(tctx.b, [c.node for c in cs])
        root, widths = cq.tapes[0], [int(w) for w in cq.widths]
        plan = native.ConjunctPlan(root, max_conjuncts=512)
        ts = TapeSet(cq.names)
        ts.pool = LocalPool(cq.consts)
        ts.tapes = [Tape(t) for t in plan.tapes]
        ct = ctx.compile(ts)
        guide = native.harvest_guide(root, cq.consts, widths, keep=True)
        tags = plan.set_ordinals(guide.set_conjuncts())
        n = K * per
        a = ctx.assignments(len(widths), n)
        b = ctx.assignments(len(widths), n)
        a.generate_guided(1, guide.arrays(), count=n)
        ctx.enable_timing(True)
        ctx.kernel_time()
        dev = {"score": [], "select": [], "mutate": []}
        wall = {"score": [], "select": [], "mutate": []}

        def timed(name, fn):
            t0 = time.perf_counter()
            out = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(ctx.kernel_time()[0])
            return out

        src, dst = a, b
        best = []
        for it in range(reps):
            timed("score", lambda: native.repair_score(rep, ct, src, row_count=n))
            el = timed("select", lambda: native.repair_select(rep, K, it))
            best.append(int(el[0]["fail_count"]))
            timed("mutate", lambda: native.repair_mutate(rep, src, dst, guide, tags, plan.col_off,
                                                         plan.cols_flat, per, seed=1,
                                                         global_base=(it + 1) * n))
            src, dst = dst, src
        ctx.enable_timing(False)
        print(json.dumps({
            "M": m, "conjuncts": plan.n, "rows": n, "elites": K, "children": per, "reps": reps,
            "device_ms_median": {k: round(statistics.median(v), 4) for k, v in dev.items()},
            "wall_ms_median": {k: round(statistics.median(v), 4) for k, v in wall.items()},
            "best_fail_count_by_iteration": best}), flush=True)
        guide.close()
        a.close()
        b.close()
        ct.close()
    rep.close()
    ctx.close()


if __name__ == "__main__":
    main()
