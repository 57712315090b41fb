"""Inputs of the mh_run partition tests (tests/test_partition_cases.py on the host,
tests/test_gpu_run_partition.py and tests/jit_rows_check.py on the device): tape sets, row windows,
tilings of the buffer, tape-range partitions, and the C oracle's results for them.

One generated buffer of N rows (``a.generate(SEED, BASE)``, run with ``index_base=BASE``): a hit in
buffer row r is reported as BASE + r by every engine, and the reference of a window (first, count)
is ``ctape.count(ts, SEED, BASE + first, count)``.

Tape sets (``tape_set(name)``):

``nv3`` / ``nv6``  24 fuzz tapes with Bool roots over three columns (pinned, asm-only variants
    reachable) or six (every column loaded), families the device already runs, so a new failure
    points at launch geometry; then one *planted* tape per mark m of MARKS, ``v0 == the value
    of column 0 in row m`` (one hit, at BASE + m: the first and last lane of a wave, both sides of
    the window edges below, the last row of the buffer); then one *planted conjunction* per mark,
    the left-nested AND (as LASER builds path conditions) of six conjuncts ``extract(v0, 4i + 3,
    4i) == nibble i of that value``: each conjunct passes about one row in 16 in every wave and
    only the AND singles the row out, which is what the conjunct-parallel parts and their combine
    kernel have to get right.
``spill``  tapes that need more than the interpreter's registers (tests/spill_cases.py) next to
    ones that fit, and planted tapes over their columns.
``big``  six fuzz tapes and the planted tapes and conjunctions of BIG_MARKS, for a buffer of
    BIG_N = 2^19 + 77 rows (the smallest at which the native kernel's waves take two chunks).
"""
import functools
import os
import random

import numpy as np

from mythril_amd.tape import Op, TapeSet
from oracle import ctape
from oracle import smt_eval as E
from tests import spill_cases as sc
from tests.fuzz import TapeFuzzer

SEED, BASE = 0x9A27, 1000
# one row more than a run with conjunct parts can hold (MH_SPLIT_ROWS = 65536), from an unaligned
# start
N = 65537 + 37
NO_HIT = 0xFFFFFFFFFFFFFFFF
THREADS = min(16, os.cpu_count() or 1)

N_FUZZ = 24
MARKS = [0, 1, 36, 37, 63, 64, 100, 101, 4132, 4133, 4134, N - 1]
N_CONJUNCTS = 6

BIG_N = (1 << 19) + 77
BIG_MARKS = [0, (1 << 19) - 1, 1 << 19, (1 << 19) + 76]
BIG_FUZZ = 6

# (first row, rows): one row at the start, inside and at the end; the last lane of a wave and the
# first of the next from unaligned starts; one-wave workgroups up to 4096 rows (sieve_kernels.hip
# kShortRows, capi.cpp MH_MERGE_ROWS) and 256-thread ones above; 65536 rows, the largest run with
# conjunct parts (MH_SPLIT_ROWS), and one more; the tail of the buffer
WINDOWS = [(0, 1), (36, 1), (N - 1, 1), (1, 63), (3, 64), (0, 65), (37, 209), (5, 257), (9, 4096),
           (7, 4097), (37, 65536), (37, 65537), (N - 64, 64), (N - 65, 65)]
RANGE_WINDOWS = [(37, 209), (7, 4097), (37, 65536)]
# of the native kernel's check with MH_JIT_ROWS_PER_WG = 512 / 1024 (tests/jit_rows_check.py): a
# partial last chunk, a last chunk clipped away, whole waves past the end
JIT_WINDOWS = [(0, 1), (3, 511), (0, 512), (5, 513), (37, 700), (9, 1089), (7, 4097)]

TILE_A = [(0, 1), (1, 36), (37, 64), (101, 4032), (4133, 4097), (8230, N - 8230)]


def _seeded_tiling():
    """About 20 windows that tile [0, N), the cuts drawn by a seeded Random; a piece of one row
    and one of 4097 rows are put in by hand."""
    rng = random.Random(SEED)
    cuts = {0, N, 777, 778, 20000, 20000 + 4097}
    while len(cuts) < 21:
        c = rng.randrange(1, N)
        if rng.random() < 0.5:
            c = min(N - 1, (c & ~63) + rng.choice((0, 1, 63)))  # on or next to a wave edge
        if c and not 20000 < c < 20000 + 4097:
            cuts.add(c)
    cuts = sorted(cuts)
    return [(lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]


TILE_B = _seeded_tiling()
TILINGS = {"tile_a": TILE_A, "tile_b": TILE_B}


def orders(tiling):
    """{name: the tiling's windows in that order}: ascending (a FIRST_HIT launch meets the minimum
    the earlier ones left), descending (each launch has to lower it), shuffled."""
    shuffled = list(tiling)
    random.Random(SEED ^ len(tiling)).shuffle(shuffled)
    return {"ascending": list(tiling), "descending": list(reversed(tiling)), "shuffled": shuffled}


def _plant(ts, b, col, n_vars, marks):
    """The planted tapes, then the planted conjunctions, of `marks` over the column node `col`."""
    values = [E.gen_assignment(SEED, n_vars, BASE + m)[0] for m in marks]
    for v in values:
        ts.add(b.finish(b.op(Op.EQ, col, b.const(v, 256))))
    for v in values:
        root = None
        for i in range(N_CONJUNCTS):
            c = b.op(Op.EQ, b.op(Op.EXTRACT, col, imm0=4 * i + 3, imm1=4 * i),
                     b.const((v >> (4 * i)) & 15, 4))
            root = c if root is None else b.op(Op.AND, root, c)
        ts.add(b.finish(root))


def _fuzz_set(nv, n_fuzz, marks):
    ts = TapeSet()
    fz = TapeFuzzer(random.Random(SEED + nv), ts, n_vars=nv, max_depth=4)
    for _ in range(n_fuzz):
        fz.tape(root_bool=True)
    _plant(ts, fz.b, fz.b.var("v0", 256), nv, marks)
    return ts


def _spill_set():
    """fan k = 13 (spills), fan k = 5 (fits), fan k = 24 (spills), a fuzz tape that spills, the fan
    k = 13 AND a nibble of x0 (a spilling tape with about one hit in 32 rows), then the planted
    tapes and conjunctions over x0."""
    names = ["x0", "x1"]
    ts = TapeSet(names)
    b = ts.builder()
    for k in (13, 5, 24):
        ts.add(b.finish(sc.fan_nodes(b, k, 1)[1]))
    _, n_ops, window = sc.fuzz_params(2)
    ts.add(b.finish(sc.fuzz_into(b, names, 2, n_ops, window, mix=True)))
    x0 = b.var("x0", 256)
    nib = b.op(Op.EQ, b.op(Op.EXTRACT, x0, imm0=3, imm1=0), b.const(9, 4))
    ts.add(b.finish(b.op(Op.AND, sc.fan_nodes(b, 13, 1)[1], nib)))
    _plant(ts, b, x0, 2, MARKS)
    return ts


SPILL_HEAD = 5  # the tapes of the spill set before its planted ones

_SETS = {
    "nv3": lambda: _fuzz_set(3, N_FUZZ, MARKS),
    "nv6": lambda: _fuzz_set(6, N_FUZZ, MARKS),
    "spill": _spill_set,
    "big": lambda: _fuzz_set(3, BIG_FUZZ, BIG_MARKS),
}
SET_NAMES = ("nv3", "nv6", "spill")


@functools.lru_cache(maxsize=None)
def tape_set(name: str) -> TapeSet:
    return _SETS[name]()


def layout(name: str):
    """(tapes before the planted ones, marks, n_tapes): the planted tape of marks[i] is tape
    head + i, its planted conjunction tape head + len(marks) + i."""
    head = {"nv3": N_FUZZ, "nv6": N_FUZZ, "spill": SPILL_HEAD, "big": BIG_FUZZ}[name]
    marks = BIG_MARKS if name == "big" else MARKS
    return head, marks, head + 2 * len(marks)


def planted(name: str):
    head, marks, _ = layout(name)
    return list(range(head, head + len(marks)))


def planted_conjunctions(name: str):
    head, marks, n = layout(name)
    return list(range(head + len(marks), n))


def tape_partitions(name: str):
    """{partition name: [(tape_first, tape_count)] covering [0, n_tapes)}: the whole set, its first
    and last tape on their own, and a cut inside the block of planted conjunctions."""
    head, marks, n = layout(name)
    cut = head + len(marks) + 5
    return {"whole": [(0, n)], "ends": [(0, 1), (1, n - 2), (n - 1, 1)],
            "cut_conjunctions": [(0, cut), (cut, n - cut)]}


@functools.lru_cache(maxsize=None)
def oracle(name: str, first: int, count: int):
    """(hit_count, first_hit), u64 per tape of set `name`, of buffer rows [first, first + count):
    the C oracle's, computed once per (set, window); read-only."""
    cnt, hit = ctape.count(tape_set(name), SEED, BASE + first, count, threads=THREADS)
    cnt.setflags(write=False)
    hit.setflags(write=False)
    return cnt, hit


def merge(results):
    """SUM of the counts and MIN of the first hits of [(hit_count, first_hit)] (NO_HIT, the
    largest u64, is MIN's identity): what launches that accumulate, or GPUs that all-reduce,
    must end with."""
    results = list(results)
    cnt = np.zeros_like(results[0][0])
    hit = np.full_like(results[0][1], NO_HIT)
    for c, h in results:
        cnt = cnt + c
        hit = np.minimum(hit, h)
    return cnt, hit


def window_oracles(name: str, windows):
    return [oracle(name, f, c) for f, c in windows]


def partial(name: str, n_rows: int = N):
    """Tapes of the set with between 1 and n_rows - 1 hits over the whole buffer."""
    cnt, _ = oracle(name, 0, n_rows)
    return [t for t in range(len(cnt)) if 0 < int(cnt[t]) < n_rows]
