"""Plain-Python restatement of the hit-listing kernels (mythril_amd/csrc/hits.hip): select, rows
and scatter.  The device tests (tests/test_gpu_hits.py) and the CPU stand-in (tests/fake_hits.py)
both compare against it.  A buffer is a list of rows, a row a list of column values (ints below
2^256), as tests/fake_device.FakeAssign keeps them."""
import numpy as np

NO_HIT = 0xFFFFFFFFFFFFFFFF
M256 = (1 << 256) - 1


def pack_masks(bools):
    """One tape's Bools of a run, in row order -> its 64-row mask words (bit r % 64 of word
    r // 64)."""
    words = [0] * ((len(bools) + 63) // 64)
    for r, v in enumerate(bools):
        if v:
            words[r >> 6] |= 1 << (r & 63)
    return words


def select(words, row_count, k, index0):
    """hits_select_kernel for one tape: (hits [k] with NO_HIT tails, n_hits, hit_count).  The
    words are walked in row order; bits at or past row_count are ignored."""
    n_words = (row_count + 63) // 64
    tail = row_count & 63
    hits, total = [], 0
    for w in range(n_words):
        m = words[w]
        if tail and w == n_words - 1:
            m &= (1 << tail) - 1
        total += bin(m).count("1")
        while m and len(hits) < k:
            low = m & -m
            hits.append(index0 + 64 * w + low.bit_length() - 1)
            m ^= low
    n = len(hits)
    return hits + [NO_HIT] * (k - n), n, total


def limbs(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def rows(table, hits, index_base, n_cols):
    """hits_rows_kernel for one tape: u32 [k, n_cols, 8], zero for a slot without a hit."""
    out = np.zeros((len(hits), n_cols, 8), dtype=np.uint32)
    for j, h in enumerate(hits):
        if h == NO_HIT:
            continue
        row = table[h - index_base]
        for c in range(n_cols):
            out[j, c] = limbs(row[c])
    return out


def scatter(table, first, cols, values):
    """scatter_kernel: values u32 [n_rows, len(cols), 8] into columns `cols` of rows first.. of
    `table`, in place; every other column keeps its content."""
    values = np.asarray(values, dtype=np.uint32).reshape(-1, len(cols), 8)
    for r in range(values.shape[0]):
        row = list(table[first + r])
        for i, c in enumerate(cols):
            row[int(c)] = sum(int(values[r, i, l]) << (32 * l) for l in range(8))
        table[first + r] = row


def run_hits(bools, table, row_first, index_base, k, n_cols):
    """mh_run_hits over bools[tape][r] = tape's Bool at buffer row row_first + r: (hits [T, k] u64,
    n_hits [T] u32, hit_count [T] u64, rows [T, k, n_cols, 8] u32)."""
    T = len(bools)
    hits = np.full((T, k), NO_HIT, dtype=np.uint64)
    nh = np.zeros(T, dtype=np.uint32)
    hc = np.zeros(T, dtype=np.uint64)
    out = np.zeros((T, k, n_cols, 8), dtype=np.uint32)
    for t in range(T):
        h, n, total = select(pack_masks(bools[t]), len(bools[t]), k, index_base + row_first)
        hits[t], nh[t], hc[t] = h, n, total
        out[t] = rows(table, h, index_base, n_cols)
    return hits, nh, hc, out
