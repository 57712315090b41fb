"""The enumerating generator on an MI355X (csrc/enumerate.hip) against decide.enumerate_rows, bit
for bit, and mh_query_enumerate against brute force over a 15015-row product.

Every comparison is exact equality of u32 limbs; no test enumerates more than 2^16 rows."""
import functools

import numpy as np
import pytest

from mythril_amd import decide, native, smt
from mythril_amd.sieve import local_tapeset
from mythril_amd.smt import And, URem, symbol_factory
from oracle import smt_eval as E

pytestmark = pytest.mark.gpu

I, L = native.DOMAIN_INTERVAL, native.DOMAIN_LIST
TOP = (1 << 256) - 1
N_COLS = 70                      # the buffer's columns; only COLS are in the domain set
COLS = [2, 17, 33, 64, 69]
WIDE = [TOP - (k * 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF) % TOP
        for k in range(5, 0, -1)]  # five ascending full-width values


def mixed():
    """Radices (3, 5, 7, 1, 11) over 5 of 70 columns: intervals whose sums carry out of limb 0
    (lo = 2^32 - 2), out of limb 1 (2^64 - 1) and end at 2^256 - 1 (2^256 - 3), a list of
    full-width values and a one-value list."""
    assert WIDE == sorted(WIDE) and len(set(WIDE)) == 5
    return native.domains_create(COLS, [I, L, I, L, I], [3, 5, 7, 1, 11],
                                 [TOP - 2, 0, (1 << 64) - 1, 0, (1 << 32) - 2],
                                 [[], WIDE, [], [TOP], []], [256] * N_COLS)


def limbs(rows, n):
    """[n][8][len(rows)] u32 of enumerate_rows' output."""
    out = np.zeros((n, 8, len(rows)), dtype=np.uint32)
    for r, row in enumerate(rows):
        for j, v in enumerate(row):
            for k in range(8):
                out[j, k, r] = (v >> (32 * k)) & 0xFFFFFFFF
    return out


def check_window(gpu_ctx, d, base, count, first=0, capacity=None):
    """Rows [first, first + count) enumerated into a buffer pre-filled by the plain generator:
    the domain columns of those rows equal the restatement, every other word keeps its
    pre-fill (the other 65 columns, and the rows outside the window)."""
    capacity = capacity or first + count + 3
    a = gpu_ctx.assignments(N_COLS, capacity)
    try:
        a.generate(0x5E17, 0)
        before = a.download(0, capacity)
        a.enumerate(d, global_base=base, first=first, count=count)
        got = a.download(0, capacity)
    finally:
        a.close()
    want = before.copy()
    want[d.cols, :, first:first + count] = limbs(decide.enumerate_rows(d, base, count), len(d.cols))
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "column %d limb %d row %d: device %#x, want %#x (%d differ)" % (
        *bad[0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_windows_match_the_restatement(gpu_ctx, count):
    """A base that is no multiple of 64, windows that cross the carries of the first three
    digits (3, 15 and 105 rows), counts around the wave and the block size."""
    d = mixed()
    try:
        assert d.rows == 1155
        check_window(gpu_ctx, d, 37, count)
        check_window(gpu_ctx, d, d.rows - count, count, first=5)  # up to the last row
    finally:
        d.close()


def test_stride_past_2_32(gpu_ctx):
    """The last column's stride is 5 * 2^40: a window near the top of the product (the whole
    product is not swept), and one across a carry into that column."""
    d = native.domains_create([0, 1, 2, 3], [I, I, L, I], [1 << 20, 1 << 20, 5, 7],
                              [(1 << 32) - 2, (1 << 64) - 1, 0, TOP - 6],
                              [[], [], WIDE, []], [256] * N_COLS)
    try:
        assert d.rows == 35 << 40
        check_window(gpu_ctx, d, d.rows - 300, 257)
        check_window(gpu_ctx, d, (5 << 40) * 3 - 100, 257)
        check_window(gpu_ctx, d, (1 << 32) - 70, 200)  # the index itself crosses 2^32
    finally:
        d.close()


def test_saturated_product_and_one_set_many_launches(gpu_ctx):
    """A product past 2^64 (rows saturate; the last column's digit is 0 everywhere), and one
    domain set used by several launches and two buffers."""
    d = native.domains_create([0, 1, 2], [I, I, I], [1 << 62, 4, 3],
                              [(1 << 64) - 1, TOP - 3, 5], [[], [], []], [256] * N_COLS)
    try:
        assert d.rows == native.ROWS_SATURATED
        for base in (0, (1 << 62) * 3 + 9, (1 << 64) - 2 - 130):
            check_window(gpu_ctx, d, base, 130)
    finally:
        d.close()


def test_invalid_arguments_launch_nothing(gpu_ctx):
    d = mixed()
    a = gpu_ctx.assignments(N_COLS, 128)
    small = gpu_ctx.assignments(COLS[-1], 128)  # lacks the set's last column
    try:
        a.generate(9, 0)
        before = a.download(0, 128)
        for kw in (dict(global_base=d.rows - 10, count=11),      # past the product
                   dict(global_base=d.rows + 1, count=0),
                   dict(global_base=0, first=100, count=29),     # past the buffer
                   dict(global_base=0, first=129, count=0)):
            with pytest.raises(native.SieveError) as e:
                a.enumerate(d, **kw)
            assert e.value.code == native.MH_E_INVALID, kw
        with pytest.raises(native.SieveError) as e:
            small.enumerate(d, global_base=0, count=10)
        assert e.value.code == native.MH_E_INVALID
        assert np.array_equal(a.download(0, 128), before)
        a.enumerate(d, global_base=d.rows, count=0)  # an empty window at the end is legal
        lib = native.load()
        assert lib.mh_assign_enumerate(None, d.h, 0, 0, 1) == native.MH_E_INVALID
        assert lib.mh_assign_enumerate(a.h, None, 0, 0, 1) == native.MH_E_INVALID
    finally:
        a.close()
        small.close()
        d.close()


# ---- mh_query_enumerate --------------------------------------------------------------------

RADICES = (3, 5, 7, 11, 13)
LOS = (250, 7, 100, 1, 0)  # 8-bit columns: 250 + 2 stays inside the width
ROWS = 3 * 5 * 7 * 11 * 13
WINDOW = 4096


@functools.lru_cache(maxsize=None)
def product_case():
    """(domains, tape set, brute force): three tapes over the 15015-row product -- its only
    model the last row, no model, several models -- and per tape the rows the oracle accepts."""
    ctx = smt.set_context(smt.Context())
    names = "abcde"
    xs = [symbol_factory.BitVecSym(n, 8) for n in names]
    c = lambda v: symbol_factory.BitVecVal(v, 8)  # noqa: E731
    last = And(*[x == c(lo + n - 1) for x, lo, n in zip(xs, LOS, RADICES)])
    none = And(xs[0] + xs[1] == c(200), xs[0] == c(LOS[0] + 1), xs[1] == c(LOS[1]))
    several = And(URem(xs[0] * xs[1] + xs[2] * xs[3] + xs[4], c(97)) == c(5), xs[3] + xs[4] == c(9))
    ts = local_tapeset(ctx.b, [t.node for t in (last, none, several)], list(names))
    d = native.domains_create(range(5), [I] * 5, RADICES, LOS, [[]] * 5, [8] * 5)
    rows = decide.enumerate_rows(d, 0, ROWS)
    pool = native._ints(ts.pool.to_array())
    hits = [[g for g, row in enumerate(rows) if E.evaluate(t.nodes, pool, row)] for t in ts.tapes]
    assert hits[0] == [ROWS - 1] and hits[1] == [] and len(hits[2]) > 3
    return d, ts, rows, hits


@pytest.mark.parametrize("tape", [0, 1, 2], ids=["last row", "none", "several"])
def test_query_enumerate_matches_brute_force(gpu_ctx, tape):
    d, ts, rows, hits = product_case()
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(5, WINDOW)
    try:
        # FIRST_HIT, window by window up to the first with a hit: the smallest row, its columns
        found = None
        for base in range(0, ROWS, WINDOW):
            n = min(WINDOW, ROWS - base)
            fh, _, out = native.query_enumerate(gpu_ctx, ct, a, d, base, n, 5, tape=tape,
                                                mode=native.MODE_FIRST_HIT)
            if int(fh[0]) != native.NO_HIT:
                found = (int(fh[0]), native._ints(out[0]))
                break
            assert not out.any()
        want = (hits[tape][0], rows[hits[tape][0]]) if hits[tape] else None
        assert found == want
        # COUNT_ALL over every window
        total, first = 0, native.NO_HIT
        for base in range(0, ROWS, WINDOW):
            n = min(WINDOW, ROWS - base)
            fh, hc, _ = native.query_enumerate(gpu_ctx, ct, a, d, base, n, 5, tape=tape,
                                               mode=native.MODE_COUNT_ALL)
            total += int(hc[0])
            first = min(first, int(fh[0]))
        assert total == len(hits[tape])
        assert first == (hits[tape][0] if hits[tape] else native.NO_HIT)
    finally:
        a.close()
        ct.close()


def test_query_enumerate_refuses_bad_arguments(gpu_ctx):
    d, ts, _, _ = product_case()
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(5, 64)
    try:
        for kw, args in ((dict(tape=3), (0, 10)),          # no such tape
                         (dict(tape=0), (0, 65)),          # past the buffer
                         (dict(tape=0), (ROWS - 5, 6)),    # past the product
                         (dict(tape=0, mode=7), (0, 10))):
            with pytest.raises(native.SieveError) as e:
                native.query_enumerate(gpu_ctx, ct, a, d, *args, 5, **kw)
            assert e.value.code == native.MH_E_INVALID, (kw, args)
    finally:
        a.close()
        ct.close()
