"""The hit-listing entry points (mh_run_hits, mh_assign_scatter, mh_query_round_hits) without a
device: their refusals come before any handle is read or any device call is made, each with its
code and a message that names the argument; and tests/hits_ref.py's select -- the restatement the
device is compared against in tests/test_gpu_hits.py -- agrees with brute force."""
import ctypes as C
import random

import numpy as np
import pytest

from mythril_amd import native
from tests import hits_ref

FAKE = C.c_void_p(1)  # not a handle: every call below must fail on its arguments first


def _run_hits(lib, ctx, ts, as_, row_count, k):
    hits = (C.c_uint64 * 64)()
    nh = (C.c_uint32 * 1)()
    return lib.mh_run_hits(ctx, ts, 0, 1, as_, 0, row_count, 0, k, hits, nh, None, 0, None)


def _round_hits(lib, ctx, ts, as_, count, k):
    hits = (C.c_uint64 * 64)()
    nh = (C.c_uint32 * 1)()
    g = native.Guide()
    return lib.mh_query_round_hits(ctx, ts, as_, C.byref(g), 1, 0, count, 0, 1, None, k, hits, nh,
                                   None, 0, None)


@pytest.mark.parametrize("call", [_run_hits, _round_hits])
def test_null_handles_are_refused(call):
    lib = native.load()
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert call(lib, *args, 64, 4) == native.MH_E_INVALID
        assert b"null" in lib.mh_last_error()


@pytest.mark.parametrize("call", [_run_hits, _round_hits])
@pytest.mark.parametrize("k", [0, 65])
def test_k_outside_its_range_is_refused(call, k):
    lib = native.load()
    assert call(lib, FAKE, FAKE, FAKE, 64, k) == native.MH_E_INVALID
    msg = lib.mh_last_error()
    assert b"k = %d" % k in msg and b"MH_HITS_MAX" in msg


@pytest.mark.parametrize("call", [_run_hits, _round_hits])
@pytest.mark.parametrize("rows", [0, 65537])
def test_row_count_outside_its_range_is_refused(call, rows):
    lib = native.load()
    assert call(lib, FAKE, FAKE, FAKE, rows, 4) == native.MH_E_INVALID
    msg = lib.mh_last_error()
    assert b"row_count = %d" % rows in msg and b"MH_HITS_MAX_ROWS" in msg


def test_scatter_refusals():
    lib = native.load()
    vals = np.zeros((2, 3, 8), dtype=np.uint32)
    for cols in ([2, 1, 3], [1, 1, 2], [0, 5, 5]):
        c = np.array(cols, dtype=np.uint32)
        assert lib.mh_assign_scatter(FAKE, 0, 2, native._ptr(c), 3,
                                     native._ptr(vals)) == native.MH_E_INVALID
        assert b"cols not strictly ascending" in lib.mh_last_error()
    c = np.array([0, 1, 2], dtype=np.uint32)
    assert lib.mh_assign_scatter(None, 0, 2, native._ptr(c), 3,
                                 native._ptr(vals)) == native.MH_E_INVALID
    assert b"null" in lib.mh_last_error()
    assert lib.mh_assign_scatter(FAKE, 0, 2, None, 3, native._ptr(vals)) == native.MH_E_INVALID
    assert b"cols" in lib.mh_last_error()


def test_constants_match_the_header():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "include", "mythril_hip.h")).read()
    assert int(re.search(r"#define MH_HITS_MAX (\d+)", text).group(1)) == native.HITS_MAX
    assert int(re.search(r"#define MH_HITS_MAX_ROWS (\d+)", text).group(1)) == native.HITS_MAX_ROWS
    assert C.sizeof(native.Spares) == 24


def _brute(bools, k, index0):
    idx = [index0 + r for r, v in enumerate(bools) if v]
    return idx[:k] + [hits_ref.NO_HIT] * (k - len(idx[:k])), min(k, len(idx)), len(idx)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_select_against_brute_force(rows, k):
    """Totals of 0, below k and above k (where the row count allows), with stale garbage in the
    last word past row_count."""
    rng = random.Random(rows * 131 + k)
    totals = sorted({0, min(rows, max(k - 1, 1)), min(rows, k), min(rows, k + 3), rows})
    for total in totals:
        on = set(rng.sample(range(rows), total))
        bools = [r in on for r in range(rows)]
        words = hits_ref.pack_masks(bools)
        if rows & 63:  # garbage at and past row_count
            words[-1] |= ((1 << 64) - 1) & ~((1 << (rows & 63)) - 1)
        index0 = rng.randrange(1 << 40)
        got = hits_ref.select(words, rows, k, index0)
        assert got == _brute(bools, k, index0), (rows, k, total)
        assert got[0] == sorted(got[0]) and len(got[0]) == k


def test_rows_and_scatter_reference():
    table = {r: [r + 1, (r << 200) | 7, 3 * r] for r in range(10)}
    vals = np.zeros((2, 2, 8), dtype=np.uint32)
    vals[0, 0, 0], vals[0, 1, 7], vals[1, 0, 1], vals[1, 1, 0] = 11, 12, 13, 14
    hits_ref.scatter(table, 4, [0, 2], vals)
    assert table[4] == [11, (4 << 200) | 7, 12 << 224] and table[5] == [13 << 32, (5 << 200) | 7, 14]
    assert table[3] == [4, (3 << 200) | 7, 9] and table[6] == [7, (6 << 200) | 7, 18]
    out = hits_ref.rows(table, [100 + 4, hits_ref.NO_HIT], 100, 2)
    assert out.shape == (2, 2, 8) and not out[1].any()
    assert out[0, 0, 0] == 11 and out[0, 1, 0] == 7 and out[0, 1, 6] == 4 << 8
