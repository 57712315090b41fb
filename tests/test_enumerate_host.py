"""decide.enumerate_rows, the restatement of the enumerating generator: over [0, rows) it visits
the cross product of the domains exactly once each, column 0 fastest, and windows concatenate."""
import itertools

import pytest

from mythril_amd import decide, native

I, L = native.DOMAIN_INTERVAL, native.DOMAIN_LIST
TOP = (1 << 256) - 1


def mixed(radices):
    """Domains of the given sizes, lists and intervals alternating, over 256-bit columns."""
    kinds, los, lists = [], [], []
    for j, n in enumerate(radices):
        if j % 2:
            kinds.append(L)
            los.append(0)
            lists.append([1000 * j + 7 * k * k for k in range(n)])
        else:
            kinds.append(I)
            los.append((1 << (40 * j)) - 1)
            lists.append([])
    return native.domains_create(list(range(len(radices))), kinds, list(radices), los, lists,
                                 [256] * len(radices))


def column_values(d, j):
    return d.lists[j] if d.kind[j] == L else [d.lo[j] + k for k in range(d.size[j])]


@pytest.mark.parametrize("radices", [(1,), (3, 5), (1, 3, 5, 7), (7, 1, 5, 3, 1), (5, 7, 3)])
def test_rows_are_the_product_once_each(radices):
    d = mixed(radices)
    rows = decide.enumerate_rows(d, 0, d.rows)
    # itertools.product varies its LAST factor fastest; the generator its first column
    want = [list(reversed(t)) for t in
            itertools.product(*[column_values(d, j) for j in reversed(range(len(radices)))])]
    assert rows == want
    assert len(set(map(tuple, rows))) == d.rows
    d.close()


def test_windows_concatenate():
    d = mixed((3, 5, 7, 1, 11))
    whole = decide.enumerate_rows(d, 0, d.rows)
    got, base = [], 0
    for n in (1, 63, 65, 257, d.rows - 386):
        got += decide.enumerate_rows(d, base, n)
        base += n
    assert base == d.rows and got == whole
    assert decide.enumerate_rows(d, 100, 0) == []
    with pytest.raises(ValueError):
        decide.enumerate_rows(d, d.rows - 1, 2)
    d.close()


def test_interval_sum_carries_and_strides_past_64_bits():
    d = native.domains_create([0, 1, 2], [I, I, I], [(1 << 62), 4, 3],
                              [(1 << 64) - 1, TOP - 3, 5], [[], [], []], [256] * 3)
    assert d.rows == native.ROWS_SATURATED  # 3 * 2^64: the last column's stride is 2^64
    g = (1 << 62) * 3 + 9
    assert decide.enumerate_rows(d, g, 1) == [[(1 << 64) - 1 + 9, TOP, 5]]
    d.close()
