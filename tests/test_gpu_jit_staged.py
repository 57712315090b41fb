"""Staged conjuncts of the tape JIT (jit.cpp emit_staged) on an MI355X: the hand-built tapes of
tests/staged_cases.py over 1 to 4 waves, and a slice of the bench's workload, short-circuit
build (staged, the default level) against the full-evaluation build and the C oracle."""
import numpy as np
import pytest

from mythril_amd import native, synth
from oracle import ctape
from tests import staged_cases as sc
from tests.test_gpu_jit import soa_of, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hand_built():
    """(tape set, 256 rows, oracle root bits [tape][row])."""
    ts, _ = sc.build()
    rows = sc.gpu_rows()
    want = np.array([[ctape.evaluate(ts, t, r) & 1 for r in rows] for t in range(len(ts.tapes))],
                    dtype=np.int64)
    return ts, rows, want


@pytest.mark.parametrize("n_rows", [64, 128, 256])
def test_hand_built_tapes(gpu_ctx, hand_built, n_rows):
    """Counts and first hits of both builds equal the C oracle's and each other's."""
    ts, rows, want = hand_built
    a = upload(gpu_ctx, soa_of(rows[:n_rows], ts.n_vars))
    w = want[:, :n_rows]
    cnt = w.sum(axis=1)
    first = np.where(cnt > 0, w.argmax(axis=1), -1)
    got = []
    for short_circuit in (True, False):
        ct = gpu_ctx.compile(ts)
        info = ct.jit(short_circuit=short_circuit)
        assert info["n_jitted"] == len(ts.tapes)
        fh, hc = native.run(gpu_ctx, ct, a, mode=native.MODE_COUNT_ALL)
        fh, hc = np.asarray(fh), np.asarray(hc).astype(np.int64)
        assert np.array_equal(hc, cnt), (short_circuit, hc.tolist(), cnt.tolist())
        hit = cnt > 0
        assert np.array_equal(fh[hit].astype(np.int64), first[hit]), (short_circuit,)
        assert all(int(f) == native.NO_HIT for f in fh[~hit])
        got.append((fh, hc))
        ct.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_config5_slice_matches_full_eval(gpu_ctx):
    """Config-5 tapes 0-255 x 2^16 generated rows: the short-circuit build at the default level
    against the full-evaluation build, identical per tape."""
    ts = synth.generate(256)
    seed, rows = synth.load_spec()["assignment_seed"], 1 << 16
    a = gpu_ctx.assignments(ts.n_vars, rows)
    a.generate(seed, 0)
    staged = gpu_ctx.compile(ts)
    staged.jit()
    full = gpu_ctx.compile(ts)
    full.jit(short_circuit=False)
    f1, c1 = native.run(gpu_ctx, staged, a, mode=native.MODE_COUNT_ALL)
    f0, c0 = native.run(gpu_ctx, full, a, mode=native.MODE_COUNT_ALL)
    assert np.array_equal(c1, c0) and np.array_equal(f1, f0)
    assert int((np.asarray(c0) > 0).sum()) > 10
