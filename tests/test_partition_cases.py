"""The inputs of the mh_run partition tests (tests/partition_cases.py), checked with the C oracle
alone: no device.  These are conditions on the inputs, not tolerances: if a change to
tests/fuzz.py or the generator ever moves them, this fails instead of the GPU tests
(tests/test_gpu_run_partition.py) silently checking less.
"""
import numpy as np
import pytest

from tests import partition_cases as pc

# partial tapes (between 1 and N - 1 hits over the buffer) per fuzz set: a little under what the
# sets gave when they were written (nv3: 17 of 24 fuzz tapes with hits, 7 partial; nv6: 21 and 19)
PARTIAL_FLOOR = {"nv3": 6, "nv6": 16}


@pytest.mark.parametrize("name", sorted(pc.TILINGS))
def test_tilings_cover_the_buffer_once(name):
    tiling = pc.TILINGS[name]
    at = 0
    for first, count in tiling:
        assert first == at and count > 0, (name, first, count)
        at += count
    assert at == pc.N
    for order in pc.orders(tiling).values():
        assert sorted(order) == sorted(tiling)


def test_seeded_tiling_shape():
    sizes = [c for _, c in pc.TILE_B]
    assert 18 <= len(sizes) <= 22 and 1 in sizes and 4097 in sizes, sizes
    orders = pc.orders(pc.TILE_B)
    assert orders["shuffled"] not in (orders["ascending"], orders["descending"])


@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_tape_partitions_cover_the_set(name):
    head, marks, n = pc.layout(name)
    assert n == len(pc.tape_set(name).tapes)
    conj = pc.planted_conjunctions(name)
    for pname, parts in pc.tape_partitions(name).items():
        at = 0
        for first, count in parts:
            assert first == at and count > 0, (pname, first, count)
            at += count
        assert at == n
    cut = pc.tape_partitions(name)["cut_conjunctions"][1][0]
    assert conj[0] < cut <= conj[-1], "the cut falls inside the planted conjunctions"


@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_merged_windows_equal_the_whole_range(name):
    """SUM of counts and MIN of first hits over TILE_A's windows are the whole buffer's, for every
    tape (the accumulation tests compare the device with the whole-range oracle)."""
    want_cnt, want_hit = pc.oracle(name, 0, pc.N)
    cnt, hit = pc.merge(pc.window_oracles(name, pc.TILE_A))
    assert np.array_equal(cnt, want_cnt) and np.array_equal(hit, want_hit)
    assert cnt.dtype == np.uint64 and hit.dtype == np.uint64


@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_planted_tapes_hit_their_mark_only(name):
    _, marks, _ = pc.layout(name)
    cnt, hit = pc.oracle(name, 0, pc.N)
    for t, m in zip(pc.planted(name), marks):
        assert int(cnt[t]) == 1 and int(hit[t]) == pc.BASE + m, (t, m)
    for t, m in zip(pc.planted_conjunctions(name), marks):
        # the AND of six nibbles: the planted row, and whatever else the oracle finds (rare)
        assert 1 <= int(cnt[t]) <= 4 and int(hit[t]) <= pc.BASE + m, (t, m, int(cnt[t]))
    # a window that ends just before a mark, or starts just after it, has no hit
    t = pc.planted(name)[marks.index(37)]
    assert int(pc.oracle(name, 0, 37)[0][t]) == 0 and int(pc.oracle(name, 0, 37)[1][t]) == pc.NO_HIT


@pytest.mark.parametrize("name", sorted(PARTIAL_FLOOR))
def test_fuzz_sets_are_not_vacuous(name):
    cnt, _ = pc.oracle(name, 0, pc.N)
    fuzz = cnt[:pc.N_FUZZ]
    with_hits = int(np.count_nonzero(fuzz))
    partial = [t for t in pc.partial(name) if t < pc.N_FUZZ]
    print("%s: %d of %d fuzz tapes have hits, %d are partial" % (name, with_hits, pc.N_FUZZ,
                                                                 len(partial)))
    assert len(partial) >= PARTIAL_FLOOR[name], (with_hits, partial)


@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_long_windows_hold_something_to_find(name):
    """Every window longer than a wave contains a planted mark or a hit of a partial tape."""
    _, marks, _ = pc.layout(name)
    partial = pc.partial(name)
    for first, count in pc.WINDOWS + pc.RANGE_WINDOWS:
        if count <= 64:
            continue
        has_mark = any(first <= m < first + count for m in marks)
        cnt, _ = pc.oracle(name, first, count)
        assert has_mark or any(int(cnt[t]) for t in partial), (first, count)


def test_spill_set_counts():
    """The spilling tapes are partial: their lanes disagree, and a wrong lane shows in the count."""
    partial = pc.partial("spill")
    assert set(range(pc.SPILL_HEAD)) <= set(partial), partial


def test_big_set_marks():
    """The set of the 2^19 + 77-row run: its marks sit on both sides of row 2^19 and on the last
    row (one window, so a few seconds of the oracle)."""
    head, marks, n = pc.layout("big")
    assert n == len(pc.tape_set("big").tapes) and marks[-1] == pc.BIG_N - 1
    cnt, hit = pc.oracle("big", (1 << 19) - 1, 78)
    for t, m in zip(pc.planted("big"), marks):
        inside = m >= (1 << 19) - 1
        assert int(cnt[t]) == int(inside) and int(hit[t]) == (pc.BASE + m if inside else pc.NO_HIT)
