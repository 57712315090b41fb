"""mh_query_round_hits_many on the device: every job's hits, n_hits, hit_count, rows_out and buffer
contents equal mh_query_round_hits' with the same arguments, bit for bit (tests/round_hits_cases.py:
one batch of 18 jobs that mixes k, spares and every shape the batch kernels treat differently, and
batches of 1 and 2); with k = 1 and no spares the results equal mh_query_round_many's in
MH_MODE_COUNT_ALL; the same parity in the C++ step() library; and the refusals that need real
handles -- host-side checks, refused before anything is queued.  The sequential entry point is
itself pinned to tests/hits_ref.py by tests/test_gpu_hits.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import native
from tests import batch_cases, lookup_cases, round_hits_cases as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    """The 18 jobs, query_round_hits' results job by job (computed once, left unchanged) and one
    batch's."""
    jobs = R.build(gpu_ctx)
    try:
        want = R.run_sequential(gpu_ctx, jobs)
        got = R.run_batched(gpu_ctx, jobs)
        yield jobs, want, got
    finally:
        R.close(jobs)


def test_batch_equals_sequential_listing_rounds(batch):
    jobs, want, got = batch
    assert len(jobs) == 18
    R.assert_equal(jobs, want, got)


def test_small_batches_and_k1_equals_the_first_hit_batch(gpu_ctx, batch):
    jobs, want, _ = batch
    for n in (1, 2):  # the smallest batches, with and without spares among them
        for lo in (0, 8):
            part = jobs[lo:lo + n]
            R.assert_equal(part, want[lo:lo + n], R.run_batched(gpu_ctx, part))
    # k = 1 without spares: mh_query_round_many's first hits, counts and rows in COUNT_ALL
    plain = [dict(j, k=1, spares=None) for j in jobs]
    listed = native.query_round_hits_many(gpu_ctx, plain)
    first = native.query_round_many(gpu_ctx, [dict(j, mode=native.MODE_COUNT_ALL) for j in plain])
    for j, (hits, nh, hc, rows), (fh, cnt, wrows) in zip(jobs, listed, first):
        assert hits.shape == (len(fh), 1) and rows.shape == (len(fh), 1) + wrows.shape[1:]
        assert np.array_equal(hits[:, 0], fh), j["name"]
        assert np.array_equal(hc, cnt), j["name"]
        assert np.array_equal(rows[:, 0], wrows), j["name"]
        assert np.array_equal(nh, (fh != native.NO_HIT).astype(np.uint32)), j["name"]


def test_the_batch_covers_what_it_names(batch):
    jobs, _, got = batch
    batch_cases.coverage(jobs[:17])  # the compiled sets are what tests/batch_cases.py names
    R.coverage(jobs, got)


def _job(ct, a, guide, count=64, n_cols=1, k=4, **kw):
    return dict(dict(tapes=ct, assign=a, guide=guide, seed=1, global_base=0, count=count,
                     n_cols=n_cols, k=k), **kw)


def _refused(ctx, jobs, code, *words):
    with pytest.raises(native.SieveError) as e:
        native.query_round_hits_many(ctx, jobs)
    assert e.value.code == code, str(e.value)
    assert "mh_query_round_hits_many: " in str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_name_the_job_and_queue_nothing(gpu_ctx):
    ts = batch_cases.one_tape_set()
    ct = gpu_ctx.compile(ts)
    g = batch_cases.HostGuide(batch_cases.flat_guide(1))
    g2 = batch_cases.HostGuide(batch_cases.flat_guide(2))
    a, b = gpu_ctx.assignments(1, 64), gpu_ctx.assignments(1, 8192)
    two = gpu_ctx.assignments(2, 64)
    other = native.Context(0)
    foreign = other.assignments(1, 64)
    lts = lookup_cases.lookup_tapeset(1, 256)
    lt = gpu_ctx.compile(lts)
    c = gpu_ctx.assignments(max(lts.n_vars, 1), 64)
    one = np.ones((1, 1, 8), dtype=np.uint32)
    try:
        good = _job(ct, a, g)
        before = native.query_round_hits_many(gpu_ctx, [good])[0]
        rows_before = a.download(0, 64)
        inval, unsup = native.MH_E_INVALID, native.MH_E_UNSUPPORTED
        _refused(gpu_ctx, [good, _job(ct, a, g)], inval, "job 1", "shares")
        _refused(gpu_ctx, [good, _job(ct, foreign, g)], inval, "job 1", "another ctx")
        _refused(gpu_ctx, [good, _job(ct, b, g, n_cols=2)], inval, "job 1", "n_cols")
        _refused(gpu_ctx, [good, _job(ct, b, g, count=4097)], unsup, "job 1", "4097")
        _refused(gpu_ctx, [_job(ct, a, g, count=65)], unsup, "job 0", "capacity")
        _refused(gpu_ctx, [good, _job(lt, c, g)], unsup, "job 1", "lookup")
        _refused(gpu_ctx, [good, _job(ct, b, g, tape_first=1, tape_count=1)], inval, "job 1")
        _refused(gpu_ctx, [good, _job(ct, b, g, count=2,
                                      spares=([0], np.ones((3, 1, 8), dtype=np.uint32)))],
                 inval, "job 1", "spares->n_rows")
        _refused(gpu_ctx, [good, _job(ct, two, g2, n_cols=2, spares=(
            [1, 0], np.ones((1, 2, 8), dtype=np.uint32)))], inval, "job 1", "ascending")
        _refused(gpu_ctx, [good, _job(ct, b, g, spares=([1], one))], inval, "job 1", "cols")
        # all-or-nothing: job 0 of a refused batch did not run (its buffer is untouched) ...
        a.generate(0xFEED, 3)
        scratch = a.download(0, 64)
        _refused(gpu_ctx, [_job(ct, a, g, seed=5, spares=([0], one)),
                           _job(ct, b, g, count=4097)], unsup, "job 1")
        assert np.array_equal(a.download(0, 64), scratch)
        # ... and the ctx still answers as before
        again = native.query_round_hits_many(gpu_ctx, [good])[0]
        assert all(np.array_equal(x, y) for x, y in zip(before, again))
        assert np.array_equal(a.download(0, 64), rows_before)
    finally:
        foreign.close()
        other.close()
        for h in (a, b, two, c, ct, lt):
            h.close()


def test_chunks_beyond_the_job_limit(gpu_ctx):
    """The wrapper chunks a list beyond MH_ROUND_MANY_MAX; a job without tapes still has its rows
    generated and its spares scattered."""
    ts = batch_cases.one_tape_set()
    ct = gpu_ctx.compile(ts)
    g = batch_cases.HostGuide(batch_cases.flat_guide(1))
    n = native.ROUND_MANY_MAX + 2
    bufs = [gpu_ctx.assignments(1, 64) for _ in range(n)]
    own = gpu_ctx.assignments(1, 64)
    try:
        jobs = [_job(ct, a, g, count=1 + i % 64, global_base=i << 8, k=1 + i % 5)
                for i, a in enumerate(bufs)]
        got = native.query_round_hits_many(gpu_ctx, jobs)
        assert len(got) == n
        for i in (0, 255, 256, n - 1):
            j = jobs[i]
            want = native.query_round_hits(gpu_ctx, ct, own, g, 1, j["global_base"], j["count"], 1,
                                           j["k"])
            assert all(np.array_equal(x, y) for x, y in zip(want, got[i])), i
        sp = ([0], np.full((2, 1, 8), 7, dtype=np.uint32))
        res = native.query_round_hits_many(
            gpu_ctx, [_job(ct, bufs[0], g, global_base=77, tape_count=0, n_cols=0, spares=sp)])[0]
        assert len(res[0]) == 0 and len(res[1]) == 0
        native.query_round_hits(gpu_ctx, ct, own, g, 1, 77, 64, 0, 4, spares=sp, tape_count=0)
        assert np.array_equal(bufs[0].download(0, 64), own.download(0, 64))
    finally:
        for a in bufs + [own]:
            a.close()
        ct.close()


def test_timing_covers_the_submission_as_one_span(gpu_ctx):
    import ctypes as C

    ts = batch_cases.tree_set()
    ct = gpu_ctx.compile(ts)
    g = batch_cases.HostGuide(batch_cases.flat_guide(3))
    bufs = [gpu_ctx.assignments(3, 256) for _ in range(4)]
    lib = gpu_ctx.lib
    try:
        ms, n = C.c_double(), C.c_uint64()
        assert lib.mh_ctx_kernel_time(gpu_ctx.h, C.byref(ms), C.byref(n)) == native.MH_OK  # drain
        assert lib.mh_ctx_enable_timing(gpu_ctx.h, 1) == native.MH_OK
        native.query_round_hits_many(
            gpu_ctx, [_job(ct, a, g, count=256, n_cols=3, global_base=i << 12)
                      for i, a in enumerate(bufs)])
        assert lib.mh_ctx_kernel_time(gpu_ctx.h, C.byref(ms), C.byref(n)) == native.MH_OK
        assert n.value == 1 and 0.0 < ms.value < 1000.0, (n.value, ms.value)
    finally:
        lib.mh_ctx_enable_timing(gpu_ctx.h, 0)
        for a in bufs:
            a.close()
        ct.close()


def test_cpp_step_library(gpu_ctx):
    """The MH_ASM_CORE=0 library's batch against its own mh_query_round_hits (one child process
    with MYTHRIL_HIP_LIB naming it: tests/noasm_round_hits_many_check.py)."""
    lib = os.path.join(ROOT, "mythril_amd", "libmythril_hip_noasm.so")
    assert os.path.exists(lib), "build it first: make -C mythril_amd/csrc noasm (build() does)"
    r = subprocess.run([sys.executable, "-u", "-m", "tests.noasm_round_hits_many_check"], cwd=ROOT,
                       env=dict(os.environ, MYTHRIL_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "noasm round_hits_many ok: 18 jobs" in r.stdout
