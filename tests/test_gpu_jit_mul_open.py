"""Open top-limb products of the tape JIT (jit.cpp op_mul_open, MH_JIT_STAGE=4) on an MI355X: the
tapes of tests/mul_open_cases.py, whole-set short-circuit builds at levels 3, 4 and unset over one
upload -- per-tape counts and first hits through mh_run against the C oracle, bit for bit: the
whole range (its last wave a partial one) and a row window off the wave boundaries with an index
base."""
import numpy as np
import pytest

from mythril_amd import native
from tests import conj_cases as cc
from tests import mul_open_cases as mc
from tests.test_gpu_jit import upload

pytestmark = pytest.mark.gpu

INDEX_BASE = 11
LEVELS = ("3", "4", None)


def expect(bits, lo, hi, base=0):
    w = bits[:, lo:hi]
    cnt = w.sum(axis=1).astype(np.uint64)
    first = np.where(cnt > 0, w.argmax(axis=1) + lo + base, native.NO_HIT).astype(np.uint64)
    return cnt, first


@pytest.mark.parametrize("n_cols", [4, 7])
def test_every_level_matches_the_oracle(gpu_ctx, monkeypatch, n_cols):
    ts, cases = mc.build(n_cols)
    rows, at = mc.gpu_rows(cases, n_cols)
    n, n_tapes = len(rows), len(ts.tapes)
    assert n_tapes <= 40 and len(at) <= 200 and n % 64 and n < 14000
    bits = np.stack([cc.root_bits(ts, t, rows) for t in range(n_tapes)])
    a = upload(gpu_ctx, cc.soa_of(rows, ts.n_vars))
    r0, r1 = 37, n - 29
    assert r0 % 64 and r1 % 64
    ids = {}
    for level in LEVELS:
        if level is None:
            monkeypatch.delenv("MH_JIT_STAGE", raising=False)
        else:
            monkeypatch.setenv("MH_JIT_STAGE", level)
        ct = gpu_ctx.compile(ts)
        info = ct.jit()
        assert info["n_jitted"] == n_tapes, (level, info)
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
        ct.close()
    a.close()
    # the open products are different code, and the default
    assert ids["3"] != ids["4"] and ids["4"] == ids[None], ids
    assert int((bits.sum(axis=1) > 0).sum()) >= n_tapes - 2
