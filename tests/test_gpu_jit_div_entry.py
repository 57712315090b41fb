"""Level-6 entries of the division subroutine (jit.cpp op_div / div_routine, MH_JIT_STAGE=6: the
raw srem entry and the run-time width dispatch) on an MI355X: the tapes of
tests/div_entry_cases.py over a thousand rows that take the raw entry's decided and undecided
sides, the dispatch into the variants and its refusals, once per level 5 and unset -- per-tape
counts and first hits through mh_run (the whole range, and a row window off the wave boundaries
with an index base) and root values through the values kernel, against the C oracle, bit for
bit."""
import numpy as np
import pytest

from mythril_amd import native
from oracle import ctape
from tests import div_entry_cases as ec
from tests.test_gpu_jit import soa_of, upload

pytestmark = pytest.mark.gpu

INDEX_BASE = 11
LEVELS = ("5", None)


@pytest.fixture(scope="module")
def case():
    """(tape set, rows, oracle values [tape][row] as ints)."""
    ts, _ = ec.build()
    rows = ec.gpu_rows()
    assert len(rows) % 64
    want = [[ctape.evaluate(ts, t, r) for r in rows] for t in range(len(ts.tapes))]
    return ts, rows, want


def expect(bits, lo, hi, base=0):
    w = bits[:, lo:hi]
    cnt = w.sum(axis=1).astype(np.uint64)
    first = np.where(cnt > 0, w.argmax(axis=1) + lo + base, native.NO_HIT).astype(np.uint64)
    return cnt, first


def test_every_level_matches_the_oracle(gpu_ctx, monkeypatch, case):
    ts, rows, want = case
    n = len(rows)
    bits = np.array([[int(v != 0) for v in w] for w in want], dtype=np.int64)
    assert int((bits.sum(axis=1) > 0).sum()) == len(ts.tapes)
    a = upload(gpu_ctx, soa_of(rows, ts.n_vars))
    r0, r1 = 37, n - 29
    assert r0 % 64 and r1 % 64
    ids = {}
    monkeypatch.delenv("MH_JIT_DIV", raising=False)
    monkeypatch.delenv("MH_JIT_ENTRY", raising=False)
    for level in LEVELS:
        if level is None:
            monkeypatch.delenv("MH_JIT_STAGE", raising=False)
        else:
            monkeypatch.setenv("MH_JIT_STAGE", level)
        ct = gpu_ctx.compile(ts)
        info = ct.jit(values=True)
        assert info["n_jitted"] == len(ts.tapes), (level, info)
        ids[level] = ct.code_id()
        cnt, first = expect(bits, 0, n)
        fh, hc = native.run(gpu_ctx, ct, a, mode=native.MODE_COUNT_ALL)
        assert np.array_equal(hc, cnt), (level, np.flatnonzero(hc != cnt).tolist())
        assert np.array_equal(fh, first), (level, np.flatnonzero(fh != first).tolist())
        fh, _ = native.run(gpu_ctx, ct, a, mode=native.MODE_FIRST_HIT)
        assert np.array_equal(fh, first), (level, np.flatnonzero(fh != first).tolist())
        cnt, first = expect(bits, r0, r1, INDEX_BASE)
        fh, hc = native.run(gpu_ctx, ct, a, row_first=r0, row_count=r1 - r0,
                            index_base=INDEX_BASE, mode=native.MODE_COUNT_ALL)
        assert np.array_equal(hc, cnt), (level, np.flatnonzero(hc != cnt).tolist())
        assert np.array_equal(fh, first), (level, np.flatnonzero(fh != first).tolist())
        vals = ct.jit_values(a)
        for t in range(len(ts.tapes)):
            got = native.limbs_to_ints(vals[t])
            bad = [r for r in range(n) if got[r] != want[t][r]]
            assert not bad, (level, t, bad[:4], hex(got[bad[0]]), hex(want[t][bad[0]]))
        ct.close()
    a.close()
    # the new entries are their own code; level 5 is not the default's
    assert ids["5"] != ids[None], ids
