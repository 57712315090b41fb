"""Random root conjunctions (tests/conj_cases.py) through the tape JIT's count path on an MI355X:
whole-set builds -- the interpreter, the full-evaluation build and the short-circuit build at
MH_JIT_STAGE 0, 1, 2 and unset -- over one upload per set, per-tape counts and first hits
against the C oracle, bit for bit: the whole range, MODE_FIRST_HIT, a row window off the wave
boundaries with an index base, and a tape window that splits the set."""
import numpy as np
import pytest

from mythril_amd import native
from tests import conj_cases as cc
from tests.test_gpu_jit import upload

pytestmark = pytest.mark.gpu

INDEX_BASE = 5
BUILDS = ("interp", "full", "0", "1", "2", None)   # MH_JIT_STAGE of the short-circuit builds


def expect(bits, lo, hi, base=0):
    """(counts, first hits) of root bits [tape][row] over rows [lo, hi); a hit is reported as
    base + its row (mh_run's global index)."""
    w = bits[:, lo:hi]
    cnt = w.sum(axis=1).astype(np.uint64)
    first = np.where(cnt > 0, w.argmax(axis=1) + lo + base, native.NO_HIT).astype(np.uint64)
    return cnt, first


def check_builds(ctx, monkeypatch, ts, rows, max_refused):
    """Every build of the set over one upload of the rows.  Returns ({build: tapes jitted}, tapes
    with a hit)."""
    n, n_tapes = len(rows), len(ts.tapes)
    bits = np.stack([cc.root_bits(ts, t, rows) for t in range(n_tapes)])
    a = upload(ctx, cc.soa_of(rows, ts.n_vars))
    r0, r1 = 37, n - 29                      # a row window off the multiples of 64
    assert r0 % 64 and r1 % 64 and r1 - r0 > 64
    t0, t1 = n_tapes // 3, n_tapes - 2       # a tape window that splits the set
    ids, jitted = {}, {}
    for build in BUILDS:
        if build in (None, "interp", "full"):
            monkeypatch.delenv("MH_JIT_STAGE", raising=False)
        else:
            monkeypatch.setenv("MH_JIT_STAGE", build)
        ct = ctx.compile(ts)
        if build != "interp":
            info = ct.jit(short_circuit=build != "full")
            jitted[build] = int(ct.jitted().sum())
            assert info["n_jitted"] == jitted[build]
            # the tapes the JIT refuses run on the interpreter inside the same mh_run
            assert n_tapes - jitted[build] <= max_refused, (build, ct.jitted().tolist())
            ids[build] = ct.code_id()
        cnt, first = expect(bits, 0, n)
        fh, hc = native.run(ctx, ct, a, mode=native.MODE_COUNT_ALL)
        assert np.array_equal(hc, cnt), (build, np.flatnonzero(hc != cnt).tolist())
        assert np.array_equal(fh, first), (build, np.flatnonzero(fh != first).tolist())
        fh, _ = native.run(ctx, ct, a, mode=native.MODE_FIRST_HIT)
        assert np.array_equal(fh, first), (build, np.flatnonzero(fh != first).tolist())
        cnt, first = expect(bits, r0, r1, INDEX_BASE)
        for mode in (native.MODE_COUNT_ALL, native.MODE_FIRST_HIT):
            fh, hc = native.run(ctx, ct, a, row_first=r0, row_count=r1 - r0,
                                index_base=INDEX_BASE, mode=mode)
            assert np.array_equal(fh, first), (build, mode, np.flatnonzero(fh != first).tolist())
            if mode == native.MODE_COUNT_ALL:
                assert np.array_equal(hc, cnt), (build, np.flatnonzero(hc != cnt).tolist())
        cnt, first = expect(bits[t0:t1], 0, n)
        fh, hc = native.run(ctx, ct, a, tape_first=t0, tape_count=t1 - t0,
                            mode=native.MODE_COUNT_ALL)
        assert np.array_equal(hc, cnt), (build, np.flatnonzero(hc != cnt).tolist())
        assert np.array_equal(fh, first), (build, np.flatnonzero(fh != first).tolist())
        cnt, first = expect(bits[t0:t1], r0, r1, INDEX_BASE)
        fh, _ = native.run(ctx, ct, a, tape_first=t0, tape_count=t1 - t0, row_first=r0,
                           row_count=r1 - r0, index_base=INDEX_BASE, mode=native.MODE_FIRST_HIT)
        assert np.array_equal(fh, first), (build, np.flatnonzero(fh != first).tolist())
        ct.close()
    a.close()
    # staging was in effect in the default build
    assert ids["0"] != ids[None], ids
    hits = int((bits.sum(axis=1) > 0).sum())
    return jitted, hits


@pytest.mark.parametrize("seed", range(4))
def test_random_conjunctions(gpu_ctx, monkeypatch, seed):
    ts, rows = cc.random_set(seed, 4 if seed % 2 == 0 else 7)
    assert len(rows) % 64
    jitted, hits = check_builds(gpu_ctx, monkeypatch, ts, rows, max_refused=2)
    print("random seed %d: jitted %s, tapes with hits %d" % (seed, jitted, hits))
    assert hits >= 8


@pytest.mark.parametrize("seed", range(4))
def test_near_ties(gpu_ctx, monkeypatch, seed):
    """Each crafted lane alone in its wave; the last wave of the upload is a partial one.  The
    value tapes of A and W stay in the set (a value tape counts the rows whose root is not 0)."""
    ts, triples, rows, _ = cc.near_tie_case(seed, 4 if seed % 2 == 0 else 7)
    rows = rows[:len(rows) - 23]
    jitted, hits = check_builds(gpu_ctx, monkeypatch, ts, rows, max_refused=0)
    print("near-tie seed %d: %d rows, jitted %s, tapes with hits %d"
          % (seed, len(rows), jitted, hits))
    assert all(v == len(ts.tapes) for v in jitted.values())
