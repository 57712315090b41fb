#!/usr/bin/env python3
"""Time of one group decided by enumeration (DESIGN §6 "Decision by enumeration") against its
rows: a group of `cols` 256-bit columns whose interval domains multiply to 2^k rows, under a
conjunction no row satisfies (so every window runs and none ends early), enumerated in windows of
the sieve's 2^16-row buffer through mh_query_enumerate, FIRST_HIT, as Sieve._decide does.

Per (cols, rows): the wall time of the whole enumeration (median of `reps` after `warm`
warm-up runs), the interpreter's share (the sieve launches' own device time,
mh_ctx_enable_timing / mh_ctx_kernel_time) and the generator's (the same windows written by
mh_assign_enumerate alone, up to a stream sync).  One JSON line each.

    python scripts/decide_cost.py [log2 rows=8,12,16,20,24] [cols=2,8,32] [reps=7] [warm=3]
"""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from mythril_amd import native, smt  # noqa: E402
from mythril_amd.sieve import local_tapeset  # noqa: E402
from mythril_amd.smt import And, symbol_factory  # noqa: E402

WINDOW = 1 << 16


def group(cols: int, log2_rows: int):
    """(tape set, domains): x_j < 2^(b_j) with the b_j summing to log2_rows, and an even sum
    equal to an odd constant, which no row satisfies."""
    ctx = smt.set_context(smt.Context())
    names = ["x%d" % j for j in range(cols)]
    xs = [symbol_factory.BitVecSym(n, 256) for n in names]
    c = lambda v: symbol_factory.BitVecVal(v, 256)  # noqa: E731
    bits = [log2_rows // cols + (1 if j < log2_rows % cols else 0) for j in range(cols)]
    acc = c(0)
    for j, x in enumerate(xs):
        acc = acc + x * c(2 * (2 * j + 3))
    root = And(acc == c(1), *[smt.ULT(x, c(1 << b)) for x, b in zip(xs, bits)])
    ts = local_tapeset(ctx.b, [root.node], names)
    d = native.domains_build(ts.tapes[0].nodes, ts.pool.to_array(), [256] * cols, range(cols))
    assert d.rows == 1 << log2_rows, (d.rows, log2_rows)
    return ts, d


def main():
    argv = sys.argv[1:]
    logs = [int(x) for x in argv[0].split(",")] if argv else [8, 12, 16, 20, 24]
    colss = [int(x) for x in argv[1].split(",")] if len(argv) > 1 else [2, 8, 32]
    reps = int(argv[2]) if len(argv) > 2 else 7
    warm = int(argv[3]) if len(argv) > 3 else 3
    ctx = native.Context(0)
    for cols in colss:
        a = ctx.assignments(max(cols, 64), WINDOW)  # the sieve's buffer: 64 columns at least
        for k in logs:
            ts, d = group(cols, k)
            ct = ctx.compile(ts)
            rows = d.rows
            wall, interp, gen = [], [], []
            for it in range(warm + reps):
                ctx.enable_timing(True)
                ctx.kernel_time()
                t0 = time.perf_counter()
                for base in range(0, rows, WINDOW):
                    fh, _, _ = native.query_enumerate(ctx, ct, a, d, base, min(WINDOW, rows - base),
                                                      cols, mode=native.MODE_FIRST_HIT)
                    assert int(fh[0]) == native.NO_HIT
                w = (time.perf_counter() - t0) * 1e3
                dev = ctx.kernel_time()[0]
                ctx.enable_timing(False)
                t0 = time.perf_counter()
                for base in range(0, rows, WINDOW):
                    a.enumerate(d, global_base=base, first=0, count=min(WINDOW, rows - base))
                ctx.synchronize()
                g = (time.perf_counter() - t0) * 1e3
                if it >= warm:
                    wall.append(w)
                    interp.append(dev)
                    gen.append(g)
            print(json.dumps({
                "cols": cols, "rows": rows, "windows": (rows + WINDOW - 1) // WINDOW,
                "reps": reps, "wall_ms_median": round(statistics.median(wall), 4),
                "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                "interpreter_device_ms_median": round(statistics.median(interp), 4),
                "generator_ms_median": round(statistics.median(gen), 4)}), flush=True)
            ct.close()
            d.close()
        a.close()
    ctx.close()


if __name__ == "__main__":
    main()
