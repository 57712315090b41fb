"""The hit-listing entry points on the device (csrc/hits.hip behind mh_run_hits, mh_assign_scatter
and mh_query_round_hits) against their CPU restatement (tests/hits_ref.py) over the oracle's Bools,
bit for bit, at the shapes where they can go wrong."""
import numpy as np
import pytest

from mythril_amd import native
from oracle import smt_eval as E
from oracle.guided_gen import generate_row
from tests import hits_cases as H
from tests import hits_ref
from tests.batch_cases import HostGuide
from tests.test_gpu_frontend import _random_guide
from tests.test_gpu_repair import native_nr_class

pytestmark = pytest.mark.gpu

BASE = (1 << 33) + 5  # index_base: global indices beyond 32 bits


@pytest.fixture(scope="module")
def listing(gpu_ctx):
    """tests/test_gpu_repair.py's tape set and rows (tests/hits_cases.py builds them) plus a tape
    that spills, compiled once, the rows uploaded once."""
    ts, soa, bools, rows = H.build()
    ct = gpu_ctx.compile(ts)
    info = ct.info()
    assert len(info) == H.N_TAPES + 1
    assert len({native_nr_class(x["n_regs"]) for x in info[:H.N_TAPES]}) >= 2
    assert any(x["features"] & 14 for x in info) and any(not x["features"] & 14 for x in info)
    assert ct.spills()[H.SPILL_TAPE] > 0 and not ct.spills()[:H.N_TAPES].any()
    # from the oracle alone: a tape with no hit, one with 1..4, one with more than 64
    totals = [x for case in H.hit_totals() for x in case]
    assert 0 in totals and any(1 <= x <= 4 for x in totals) and any(x > 64 for x in totals)
    a = gpu_ctx.assignments(3, H.N_ROWS)
    a.upload(soa)
    yield ct, a, bools, rows, soa
    a.close()
    ct.close()


@pytest.mark.parametrize("tape_first,tape_count,row_first,row_count,k", H.CASES)
def test_run_hits_matches_reference(gpu_ctx, listing, tape_first, tape_count, row_first, row_count,
                                    k):
    ct, a, bools, rows, _ = listing
    got = native.run_hits(gpu_ctx, ct, a, k, 3, tape_first=tape_first, tape_count=tape_count,
                          row_first=row_first, row_count=row_count, index_base=BASE)
    want = hits_ref.run_hits(bools(tape_first, tape_count, row_first, row_count), rows, row_first,
                             BASE, k, 3)
    for g, w, what in zip(got, want, ("hits", "n_hits", "hit_count", "rows")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w), what
    hits, nh, hc, out = got
    assert np.array_equal(nh, np.minimum(hc, k))
    for t in range(tape_count):  # MH_NO_HIT and zero tails
        assert (hits[t, int(nh[t]):] == native.NO_HIT).all() and not out[t, int(nh[t]):].any()


@pytest.mark.parametrize("tape_first,tape_count,row_first,row_count,k", H.CASES)
def test_k1_equals_run_rows(gpu_ctx, listing, tape_first, tape_count, row_first, row_count, k):
    ct, a, _, _, _ = listing
    kw = dict(tape_first=tape_first, tape_count=tape_count, row_first=row_first,
              row_count=row_count, index_base=BASE)
    hits, nh, hc, out = native.run_hits(gpu_ctx, ct, a, 1, 3, **kw)
    fh, cnt, rows = native.run_rows(gpu_ctx, ct, a, 3, mode=native.MODE_COUNT_ALL, **kw)
    assert np.array_equal(hits[:, 0], fh) and np.array_equal(hc, cnt)
    assert np.array_equal(out[:, 0], rows)
    assert np.array_equal(nh, (fh != native.NO_HIT).astype(np.uint32))


@pytest.mark.parametrize("first,n_rows,cols", [(0, 1, [1]), (61, 5, [0, 2]),
                                               (4095, 64, [0, 1, 2])])
def test_scatter_matches_reference(gpu_ctx, listing, first, n_rows, cols):
    _, _, _, rows, soa = listing
    rng = np.random.default_rng(first + n_rows)
    vals = rng.integers(0, 1 << 32, size=(n_rows, len(cols), 8), dtype=np.uint64).astype(np.uint32)
    a = gpu_ctx.assignments(3, H.N_ROWS)
    try:
        a.upload(soa)
        a.scatter(first, cols, vals)
        got = a.download(0, H.N_ROWS)
    finally:
        a.close()
    table = {r: list(rows[r]) for r in range(H.N_ROWS)}
    hits_ref.scatter(table, first, cols, vals)
    want = soa.copy()
    for r in range(first, first + n_rows):
        for c in range(3):
            want[c, :, r] = hits_ref.limbs(table[r][c])
    assert np.array_equal(got, want)
    assert not np.array_equal(got, soa)


def test_scatter_of_nothing_and_refusals(gpu_ctx, listing):
    _, a, _, _, soa = listing
    a.scatter(0, [], np.zeros((3, 0, 8), dtype=np.uint32))
    a.scatter(7, [0, 1], np.zeros((0, 2, 8), dtype=np.uint32))
    assert np.array_equal(a.download(0, 64), soa[:, :, :64])
    one = np.zeros((1, 1, 8), dtype=np.uint32)
    with pytest.raises(native.SieveError, match="cols beyond"):
        a.scatter(0, [3], one)
    with pytest.raises(native.SieveError, match="capacity"):
        a.scatter(H.N_ROWS, [0], one)
    ct = listing[0]
    with pytest.raises(native.SieveError, match="n_cols"):
        native.run_hits(gpu_ctx, ct, a, 4, 4, row_count=64)
    with pytest.raises(native.SieveError, match="row range"):
        native.run_hits(gpu_ctx, ct, a, 4, 3, row_first=H.N_ROWS - 10, row_count=64)


def _guide(seed):
    arrays = _random_guide(np.random.default_rng(seed), 3, 20)
    arrays["width"][:] = [256, 64, 256]
    return arrays, HostGuide(arrays)


@pytest.mark.parametrize("count", [4096, 130])
def test_round_hits_without_spares_is_query_round(gpu_ctx, listing, count):
    """spares=None, k=1: the outputs and the buffer's contents of mh_query_round(COUNT_ALL)."""
    ct = listing[0]
    _, guide = _guide(count)
    a1 = gpu_ctx.assignments(3, 4096)
    a2 = gpu_ctx.assignments(3, 4096)
    try:
        fh, cnt, rows = native.query_round(gpu_ctx, ct, a1, guide, 0xABCD, BASE, count, 3,
                                           mode=native.MODE_COUNT_ALL)
        hits, nh, hc, out = native.query_round_hits(gpu_ctx, ct, a2, guide, 0xABCD, BASE, count,
                                                    3, 1)
        assert np.array_equal(hits[:, 0], fh) and np.array_equal(hc, cnt)
        assert np.array_equal(out[:, 0], rows)
        assert np.array_equal(a1.download(0, count), a2.download(0, count))
        assert cnt.any()
    finally:
        a1.close()
        a2.close()


@pytest.mark.parametrize("count", [4096, 130])
def test_round_hits_with_spares(gpu_ctx, listing, count):
    """3 spare rows over 2 of 3 columns: the buffer is the guided generator's rows
    (oracle/guided_gen.py) with the scatter applied, the hits hits_ref's over it."""
    ct = listing[0]
    ts = H.build()[0]
    arrays, guide = _guide(1000 + count)
    seed, k, tf, tc = 0x5EED, 5, 0, 7
    rng = np.random.default_rng(count)
    vals = rng.integers(0, 1 << 32, size=(3, 2, 8), dtype=np.uint64).astype(np.uint32)
    vals[0, 0, 1:] = 0  # (a small v0: the short tapes' comparisons hold on the first spare)
    vals[0, 0, 0] = 5
    a = gpu_ctx.assignments(3, 4096)
    try:
        got = native.query_round_hits(gpu_ctx, ct, a, guide, seed, BASE, count, 3, k,
                                      spares=([0, 2], vals), tape_first=tf, tape_count=tc)
        buf = a.download(0, count)
    finally:
        a.close()
    table = {r: generate_row(seed, BASE + r, arrays) for r in range(count)}
    hits_ref.scatter(table, 0, [0, 2], vals)
    for r in range(count):
        for c in range(3):
            assert buf[c, :, r].tolist() == hits_ref.limbs(table[r][c]), (r, c)
    bools = [[bool(E.evaluate(ts.tapes[t].nodes, ts.pool.values, table[r])) for r in range(count)]
             for t in range(tf, tf + tc)]
    want = hits_ref.run_hits(bools, table, 0, BASE, k, 3)
    for g, w, what in zip(got, want, ("hits", "n_hits", "hit_count", "rows")):
        assert np.array_equal(g, w), what
    assert int(got[0][0, 0]) == BASE  # tape 0 (v0 < 8) is answered by the first spare row
    assert (got[1] > 0).any()


def test_one_submission_is_one_span(gpu_ctx, listing):
    """With timing enabled a listing run and a listing round are one span each; the values-path
    launch counter (mh_ctx_eval_launches) is untouched."""
    ct, a, _, _, _ = listing
    _, guide = _guide(9)
    a2 = gpu_ctx.assignments(3, 4096)
    before = native.eval_launches(gpu_ctx)
    gpu_ctx.enable_timing(True)
    try:
        gpu_ctx.kernel_time()
        native.run_hits(gpu_ctx, ct, a, 64, 3, row_first=5, row_count=257)
        ms, n = gpu_ctx.kernel_time()
        assert n == 1 and ms > 0
        vals = np.ones((2, 1, 8), dtype=np.uint32)
        native.query_round_hits(gpu_ctx, ct, a2, guide, 1, 0, 4096, 3, 8, spares=([1], vals))
        ms, n = gpu_ctx.kernel_time()
        assert n == 1 and ms > 0
    finally:
        gpu_ctx.enable_timing(False)
        a2.close()
    assert native.eval_launches(gpu_ctx) == before
