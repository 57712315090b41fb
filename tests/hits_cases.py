"""The host side of the hit-listing device tests (tests/test_gpu_hits.py): the tape set of
tests/test_gpu_repair.py's scoring fixture -- 133 fuzzed Bool tapes over 3 columns -- plus one tape
that spills, 4200 edge-biased rows, the tested (tape, row) ranges, and a memo of the oracle's
Bools.  No device is needed to build it; the device test's fixture asserts the hit distribution
it relies on (hit_totals)."""
import random

from mythril_amd.tape import Op, TapeSet
from oracle import smt_eval as E
from tests.fuzz import TapeFuzzer, assignment_soa, soa_row, tree_tape
from tests.spill_cases import fan_nodes

N_TAPES, N_ROWS = 133, 4200
SPILL_TAPE = N_TAPES  # the fan of tests/spill_cases.py over v0, v1: more live values than registers

# (tape_first, tape_count, row_first, row_count, k): the 64-tape LDS chunk, the one-wave (<= 4096
# rows) and 256-thread workgroup forms, partial last waves, row_first != 0; then the spilled tape
CASES = [(0, 2, 0, 1, 1), (1, 64, 1, 63, 4), (0, 64, 3, 64, 64), (3, 65, 0, 65, 5),
         (0, 130, 5, 257, 64), (130, 2, 7, 4097, 3), (66, 3, 100, 4100, 64),
         (SPILL_TAPE, 1, 3, 130, 5)]

_built = []


def build():
    """(tape set, soa u32 [3, 8, N_ROWS], bools(tape_first, tape_count, row_first, row_count) ->
    [tape][row] from the oracle, memoised, rows as lists of column values); built once."""
    if _built:
        return _built[0]
    rng = random.Random(0x5C0)
    ts = TapeSet()
    fz = TapeFuzzer(rng, ts, n_vars=3, allow_keccak=False, max_depth=4)
    b = fz.b
    for i in range(N_TAPES):
        if i % 16 == 5:    # 8 registers: the middle class
            tree_tape(ts, b, 5, i)
        elif i % 32 == 9:  # 10 registers: the largest class
            tree_tape(ts, b, 7, i)
        elif i % 3 == 0:  # short tapes: few registers, no complex op
            v = b.var("v%d" % (i % 3), 256)
            ts.add(b.finish(b.op(Op.BVULT, v, b.const(1 << (8 * (i % 31) + 3), 256))))
        else:
            fz.max_depth = 1 + i % 4
            fz.tape(root_bool=True)
    ts.add(b.finish(fan_nodes(b, 13, 1, var=lambda n, w: b.var("v" + n[1:], w))[1]))
    soa = assignment_soa(rng, 3, N_ROWS)
    rows = [soa_row(soa, r) for r in range(N_ROWS)]
    memo = {}

    def bools(tape_first, tape_count, row_first, row_count):
        out = []
        for t in range(tape_first, tape_first + tape_count):
            line = []
            for r in range(row_first, row_first + row_count):
                if (t, r) not in memo:
                    memo[t, r] = bool(E.evaluate(ts.tapes[t].nodes, ts.pool.values, rows[r]))
                line.append(memo[t, r])
            out.append(line)
        return out

    _built.append((ts, soa, bools, rows))
    return _built[0]


def hit_totals():
    """Per case, each tape's hit count in the case's rows (the oracle alone)."""
    _, _, bools, _ = build()
    return [[sum(line) for line in bools(tf, tc, rf, rc)] for tf, tc, rf, rc, _ in CASES]
