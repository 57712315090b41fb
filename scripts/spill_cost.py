#!/usr/bin/env python3
"""What a spill costs: a 4096-row interpreter round of the fan tape (tests/spill_cases.py) that
just fits the 15 registers (k = 12) against fans that spill (k = 13, 16, 24).

Per fan: 3 warm-up and 7 timed mh_run calls over 4096 generated rows (one-wave workgroups, the
shape of a query's first round), host wall time around the blocking call; median, min and max in
microseconds, the tape's instruction slots and its D_SPILL / D_FILL counts.  The fans differ by
more than their spill code (every value adds its own chain and two terms), so the price of a pair
is read off the spilling fans alone: the slope of the median over the pair count between k = 13
and k = 24, less the slope of the fitting fans k = 10 .. 12 over their values, which prices a
value's own instructions.

    python scripts/spill_cost.py            # prints one JSON line per fan and a summary line
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, WARMUP, TIMED = 4096, 3, 7


def spill_counts(words):
    """(D_SPILL, D_FILL) instructions of a one-tape word list: the slots walked as the
    interpreter walks them (op numbers out of dev_isa.h), so an inline constant is never taken
    for an instruction."""
    from tests.spill_cases import spill_ops

    ops = [name for _, name, _, _ in spill_ops(words)]
    return ops.count("D_SPILL"), ops.count("D_FILL")


def main() -> int:
    try:
        import torch

        torch.cuda.init()
    except Exception:  # noqa: BLE001 - the library initialises HIP itself then
        pass
    from mythril_amd import native
    from tests import spill_cases as sc
    emu = sc.SpillEmulator()
    ctx = native.Context(0)
    out = []
    try:
        for k in (10, 11, 12, 13, 16, 24):
            ts = sc.fan(k, 1)
            words = emu.words(ts)
            n_spill, n_fill = spill_counts(words)
            ct = ctx.compile(ts)
            a = ctx.assignments(2, ROWS)
            a.generate(0x5EED, 0)
            times = []
            for i in range(WARMUP + TIMED):
                t0 = time.perf_counter()
                native.run(ctx, ct, a, mode=native.MODE_COUNT_ALL)
                dt = (time.perf_counter() - t0) * 1e6
                if i >= WARMUP:
                    times.append(dt)
            rec = dict(k=k, slots=len(words) // 2, spill_slots=int(ct.spills()[0]),
                       d_spill=n_spill, d_fill=n_fill, median_us=round(statistics.median(times), 1),
                       min_us=round(min(times), 1), max_us=round(max(times), 1))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            a.close()
            ct.close()
    finally:
        ctx.close()
    by = {r["k"]: r for r in out}
    per_value = (by[12]["median_us"] - by[10]["median_us"]) / 2.0
    pairs = by[24]["d_fill"] - by[13]["d_fill"]
    slope = (by[24]["median_us"] - by[13]["median_us"]) / (24 - 13)
    per_pair = (slope - per_value) * (24 - 13) / max(pairs, 1)
    print(json.dumps(dict(rows=ROWS, us_per_value_that_fits=round(per_value, 2),
                          us_per_value_that_spills=round(slope, 2),
                          fills_k13_to_k24=pairs, us_per_spill_fill_pair=round(per_pair, 2),
                          first_spill_us=round(by[13]["median_us"] - by[12]["median_us"]
                                               - per_value, 2))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
