"""The candidate generators on an MI355X against the oracle, bit for bit on EVERY generated row:
mh_assign_generate_guided in each of its three kernels (staged LDS, LDS, plain: generate.hip
launch_generate_guided; tests/guide_cases.py names a guide or more per form and
tests/test_guide_cases.py shows on the CPU which form each takes), value sets resolved in LDS
with many collisions, row windows that leave every other row alone, launches split differently,
copy entries at their limb and width edges, indices past 2^32 and seeds with the top bit set; and
the plain generator mh_assign_generate over a row count that is no multiple of its block.

Every comparison is exact equality of u32 limbs.
"""
import functools

import numpy as np
import pytest

from mythril_amd import native
from oracle import smt_eval
from tests import guide_cases as gc

pytestmark = pytest.mark.gpu

PAST_2_32 = (1 << 32) - 100  # global_base + row crosses 2^32 inside a 200-row launch


@functools.lru_cache(maxsize=None)
def _oracle(name, seed, base, rows):
    """The oracle's rows [0, rows) of a named guide, computed once and left unchanged."""
    guide = gc.directed_copy_guide() if name == "directed" else gc.guide(name)
    want = gc.oracle_rows(seed, base, guide, range(rows))
    want.setflags(write=False)
    return want


def _mismatch(got, want, first=0):
    """None, or (column, limb, row) of the first differing limb."""
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    v, k, r = (int(x) for x in bad[0])
    return "column %d limb %d row %d: device %#x, oracle %#x (%d limbs differ)" % (
        v, k, first + r, int(got[v, k, r]), int(want[v, k, r]), len(bad))


def _check_against_oracle(gpu_ctx, name, arrays, seed, base, rows):
    """Rows [0, rows) generated into a buffer two columns wider than the guide and pre-filled by
    the plain generator: every guide column of every row equals the oracle, the two extra
    columns keep their pre-fill."""
    n_cols = len(arrays["width"])
    a = gpu_ctx.assignments(n_cols + 2, rows)
    try:
        a.generate(1, 0)
        before = a.download(0, rows)
        a.generate_guided(seed, arrays, global_base=base, first=0, count=rows)
        got = a.download(0, rows)
    finally:
        a.close()
    assert np.array_equal(got[n_cols:], before[n_cols:]), "columns past the guide were written"
    assert _mismatch(got[:n_cols], _oracle(name, seed, base, rows)) is None, \
        (name, gc.generator_form(arrays), _mismatch(got[:n_cols], _oracle(name, seed, base, rows)))


@pytest.mark.parametrize("name", gc.FORM_CASES + gc.ALL_VALUE_CASES + gc.COPY_FIRST_CASES)
def test_every_form_matches_oracle(gpu_ctx, name):
    """Each kernel form (the case's name says which), mixed, all-value and copy-first guides: 200
    rows (a partial last 64-row block), the global index crossing 2^32 inside the launch."""
    arrays = gc.guide(name)
    assert gc.generator_form(arrays) == gc.CASES[name][1]
    _check_against_oracle(gpu_ctx, name, arrays, 0xABCD + len(arrays["width"]), PAST_2_32, 200)


def test_value_set_collisions(gpu_ctx):
    """5 columns, 400 value-only sets, 256 rows: each of the 16 waves walks 25 sets and every
    [column][row] slot takes many atomic max updates; the largest applied entry must win."""
    arrays = gc.guide(gc.COLLISION_CASE)
    assert gc.leading_value_sets(arrays) == 400 and gc.generator_form(arrays) == "staged"
    _check_against_oracle(gpu_ctx, gc.COLLISION_CASE, arrays, 0xC0111DE, PAST_2_32, 256)


WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (1, 64), (63, 2), (64, 64), (100, 200), (37, 603),
           (0, 0), (640, 0), (200, 0)]


@pytest.mark.parametrize("name", gc.SMALL_CASES)
def test_row_windows(gpu_ctx, name):
    """Rows [first, first + count) of a 640-row buffer: inside the window the oracle's row
    global_base + row, outside it the pre-fill, bit for bit; count = 0 changes nothing."""
    arrays = gc.guide(name)
    assert gc.generator_form(arrays) == gc.CASES[name][1]
    n_cols, rows, seed, base = len(arrays["width"]), 640, 0x5EED0 + len(name), (1 << 32) - 300
    want = _oracle(name, seed, base, rows)
    a = gpu_ctx.assignments(n_cols + 2, rows)
    try:
        a.generate(1, 0)
        prefill = a.download(0, rows)
        for first, count in WINDOWS:
            a.generate(1, 0)  # a fresh pre-fill per window
            a.generate_guided(seed, arrays, global_base=base, first=first, count=count)
            got = a.download(0, rows)
            inside = np.zeros(rows, dtype=bool)
            inside[first:first + count] = True
            assert np.array_equal(got[:, :, ~inside], prefill[:, :, ~inside]), \
                (name, first, count, "rows outside the window changed")
            assert np.array_equal(got[n_cols:], prefill[n_cols:]), (name, first, count)
            assert _mismatch(got[:n_cols, :, inside], want[:, :, inside], first) is None, \
                (name, first, count,
                 _mismatch(got[:n_cols, :, inside], want[:, :, inside], first))
    finally:
        a.close()


@pytest.mark.parametrize("name", gc.SMALL_CASES)
def test_launch_geometry_independence(gpu_ctx, name):
    """Rows [0, 4096) in one call and as [0, 77) + [77, 1000) + [1000, 4096) into a second
    buffer: the same bits (a row's value depends on global_base + row alone, not on the launch
    that writes it).  The device's output alone, compared whole."""
    arrays = gc.guide(name)
    n_cols, rows, seed, base = len(arrays["width"]), 4096, 0x6E0 + len(name), (1 << 32) - 2000
    one = gpu_ctx.assignments(n_cols, rows)
    parts = gpu_ctx.assignments(n_cols, rows)
    try:
        one.generate(1, 0)
        parts.generate(2, 0)
        one.generate_guided(seed, arrays, global_base=base, first=0, count=rows)
        for first, end in ((0, 77), (77, 1000), (1000, 4096)):
            parts.generate_guided(seed, arrays, global_base=base, first=first, count=end - first)
        got_one, got_parts = one.download(0, rows), parts.download(0, rows)
    finally:
        one.close()
        parts.close()
    assert _mismatch(got_parts, got_one) is None, (name, _mismatch(got_parts, got_one))
    # and not the pre-fill: the first rows against the oracle
    assert np.array_equal(got_one[:, :, :8], gc.oracle_rows(seed, base, arrays, range(8)))


def test_directed_copy_edges(gpu_ctx):
    """tests/guide_cases.py directed_copy_guide: one copy entry per set at the edge offsets and
    bit counts, limb-aligned and not, past bit 256, src == dst, narrow destinations, a chain."""
    arrays = gc.directed_copy_guide()
    _check_against_oracle(gpu_ctx, "directed", arrays, 0xD1EC7ED, (1 << 32) - 64, 128)


def test_random_copy_guide_full_range(gpu_ctx):
    """Copy sets only (copy_p = 1), offsets 0..255 and 1..256 bits, 9 columns, 60 sets."""
    arrays = gc.guide("copies_9x60")
    assert np.all(arrays["entry_col"] & 0x80000000)
    _check_against_oracle(gpu_ctx, "copies_9x60", arrays, 0xC0B1E5, PAST_2_32, 200)


INDEX_BASES = [0, (1 << 32) - 1, (1 << 63) + 12345]
INDEX_SEEDS = [0, (1 << 64) - 1, 0x8000000000000001]


@pytest.mark.parametrize("seed", INDEX_SEEDS, ids=lambda s: "seed%#x" % s)
@pytest.mark.parametrize("base", INDEX_BASES, ids=lambda b: "base%#x" % b)
def test_large_indices_and_seeds(gpu_ctx, base, seed):
    """A small guide at global bases 0, 2^32 - 1 and 2^63 + 12345 with seeds 0, 2^64 - 1 and one
    with only its top and bottom bits set: 64 rows each.  The oracle's gen_limb is first checked
    against the library's host mh_gen_limb at these arguments (both reduce modulo 2^64)."""
    from oracle.guided_gen import SALT_MODE, SALT_SET

    for salt in (0, SALT_MODE, SALT_SET):
        for row in (0, 1, 63):
            for var, limb in ((0, 0), (6, 7), (59, 0)):
                assert native.gen_limb(seed ^ salt, var, base + row, limb) == \
                    smt_eval.gen_limb(seed ^ salt, var, base + row, limb)
    name = "small_staged_7x60"
    _check_against_oracle(gpu_ctx, name, gc.guide(name), seed, base, 64)


def test_plain_generator_every_row(gpu_ctx):
    """mh_assign_generate over 1000 rows (no multiple of its 256-row block) of 4 columns from
    base 2^32 - 500: every row and limb against smt_eval.gen_limb."""
    seed, base, rows, n_cols = 0x9E3779B97F4A7C15, (1 << 32) - 500, 1000, 4
    a = gpu_ctx.assignments(n_cols, rows)
    try:
        a.generate(seed, base)
        got = a.download(0, rows)
    finally:
        a.close()
    want = np.array([[[smt_eval.gen_limb(seed, v, base + r, k) for r in range(rows)]
                      for k in range(8)] for v in range(n_cols)], dtype=np.uint32)
    assert _mismatch(got, want) is None, _mismatch(got, want)
    for v, k, r in ((0, 0, 0), (3, 7, rows - 1), (2, 5, 500)):  # the library's host restatement
        assert native.gen_limb(seed, v, base + r, k) == int(got[v, k, r])
