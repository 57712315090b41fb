"""mh_query_round_many on the device: every job's first_hit, hit_count, rows_out and buffer
contents equal mh_query_round's with the same arguments, bit for bit (tests/batch_cases.py: one
batch of 17 jobs over every shape the batch kernels treat differently, and batches of 1 and 2);
the same in the C++ step() library; timing spans; and the refusals that need real handles --
host-side checks, refused before anything is queued, so nothing is launched with bad arguments."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import native
from tests import batch_cases, lookup_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_equals_sequential_rounds(gpu_ctx):
    line = batch_cases.check(gpu_ctx)
    assert line.startswith("round_many ok: 17 jobs")


def test_cpp_step_library(gpu_ctx):
    """The MH_ASM_CORE=0 library's batch kernel against its own mh_query_round (one child process
    with MYTHRIL_HIP_LIB naming it: tests/noasm_round_many_check.py)."""
    lib = os.path.join(ROOT, "mythril_amd", "libmythril_hip_noasm.so")
    assert os.path.exists(lib), "build it first: make -C mythril_amd/csrc noasm (build() does)"
    r = subprocess.run([sys.executable, "-u", "-m", "tests.noasm_round_many_check"], cwd=ROOT,
                       env=dict(os.environ, MYTHRIL_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "noasm round_many ok: 17 jobs" in r.stdout


def _job(ct, a, guide, count=64, n_cols=1, **kw):
    return dict(dict(tapes=ct, assign=a, guide=guide, seed=1, global_base=0, count=count,
                     n_cols=n_cols), **kw)


def _refused(ctx, jobs, code, *words):
    with pytest.raises(native.SieveError) as e:
        native.query_round_many(ctx, jobs)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals_name_the_job_and_queue_nothing(gpu_ctx):
    ts = batch_cases.one_tape_set()
    ct = gpu_ctx.compile(ts)
    g = batch_cases.HostGuide(batch_cases.flat_guide(1))
    a, b = gpu_ctx.assignments(1, 64), gpu_ctx.assignments(1, 8192)
    other = native.Context(0)
    foreign = other.assignments(1, 64)
    lts = lookup_cases.lookup_tapeset(1, 256)
    lt = gpu_ctx.compile(lts)
    c = gpu_ctx.assignments(max(lts.n_vars, 1), 64)
    try:
        good = _job(ct, a, g)
        before = native.query_round_many(gpu_ctx, [good])[0]
        rows_before = a.download(0, 64)
        inval, unsup = native.MH_E_INVALID, native.MH_E_UNSUPPORTED
        _refused(gpu_ctx, [good, _job(ct, a, g)], inval, "job 1", "shares")
        _refused(gpu_ctx, [good, _job(ct, foreign, g)], inval, "job 1", "another ctx")
        _refused(gpu_ctx, [good, _job(ct, b, g, n_cols=2)], inval, "job 1", "n_cols")
        _refused(gpu_ctx, [good, _job(ct, b, g, count=4097)], unsup, "job 1", "4097")
        _refused(gpu_ctx, [_job(ct, a, g, count=65)], unsup, "job 0", "capacity")
        _refused(gpu_ctx, [good, _job(lt, c, g)], unsup, "job 1", "lookup")
        _refused(gpu_ctx, [good, _job(ct, b, g, tape_first=1, tape_count=1)], inval, "job 1")
        _refused(gpu_ctx, [good, _job(ct, b, g, mode=7)], inval, "job 1", "mode")
        # all-or-nothing: job 0 of a refused batch did not run (its buffer is untouched) ...
        a.generate(0xFEED, 3)
        scratch = a.download(0, 64)
        _refused(gpu_ctx, [_job(ct, a, g, seed=5), _job(ct, b, g, count=4097)], unsup, "job 1")
        assert np.array_equal(a.download(0, 64), scratch)
        # ... and the ctx still answers as before
        again = native.query_round_many(gpu_ctx, [good])[0]
        assert all(np.array_equal(x, y) for x, y in zip(before, again))
        assert np.array_equal(a.download(0, 64), rows_before)
    finally:
        foreign.close()
        other.close()
        for h in (a, b, c, ct, lt):
            h.close()


def test_chunks_beyond_the_job_limit_and_empty_jobs(gpu_ctx):
    """The wrapper chunks a list beyond MH_ROUND_MANY_MAX; the library refuses it whole.  A job
    without tapes or rows is legal and still has its rows generated."""
    ts = batch_cases.one_tape_set()
    ct = gpu_ctx.compile(ts)
    g = batch_cases.HostGuide(batch_cases.flat_guide(1))
    n = native.ROUND_MANY_MAX + 3
    bufs = [gpu_ctx.assignments(1, 64) for _ in range(n)]
    try:
        jobs = [_job(ct, a, g, count=1 + i % 64, global_base=i << 8, mode=native.MODE_COUNT_ALL)
                for i, a in enumerate(bufs)]
        arr = (native.RoundJob * n)()
        assert gpu_ctx.lib.mh_query_round_many(gpu_ctx.h, arr, n) == native.MH_E_INVALID
        assert b"MH_ROUND_MANY_MAX" in gpu_ctx.lib.mh_last_error()
        got = native.query_round_many(gpu_ctx, jobs)
        assert len(got) == n
        for i in (0, 1, 255, 256, n - 1):
            j = jobs[i]
            fh, hc, rows = native.query_round(gpu_ctx, ct, j["assign"], g, 1, j["global_base"],
                                              j["count"], 1, mode=native.MODE_COUNT_ALL)
            assert np.array_equal(fh, got[i][0]) and np.array_equal(hc, got[i][1])
            assert np.array_equal(rows, got[i][2])
        # no tapes: the generator still writes the rows, as mh_query_round's does
        a = bufs[0]
        a.generate(9, 9)
        fh, hc, rows = native.query_round_many(
            gpu_ctx, [_job(ct, a, g, count=64, global_base=77, tape_count=0, n_cols=0)])[0]
        assert len(fh) == 0 and len(hc) == 0
        got_rows = a.download(0, 64)
        native.query_round(gpu_ctx, ct, a, g, 1, 77, 64, 0, tape_count=0)
        assert np.array_equal(a.download(0, 64), got_rows)
        # no rows
        fh, hc, _ = native.query_round_many(gpu_ctx, [_job(ct, a, g, count=0)])[0]
        assert fh.tolist() == [native.NO_HIT] and hc.tolist() == [0]
    finally:
        for a in bufs:
            a.close()
        ct.close()


def test_timing_covers_the_submission_as_one_span(gpu_ctx):
    ts = batch_cases.tree_set()
    ct = gpu_ctx.compile(ts)
    g = batch_cases.HostGuide(batch_cases.flat_guide(3))
    bufs = [gpu_ctx.assignments(3, 256) for _ in range(4)]
    lib = gpu_ctx.lib
    try:
        ms, n = C.c_double(), C.c_uint64()
        assert lib.mh_ctx_kernel_time(gpu_ctx.h, C.byref(ms), C.byref(n)) == native.MH_OK  # drain
        assert lib.mh_ctx_enable_timing(gpu_ctx.h, 1) == native.MH_OK
        native.query_round_many(gpu_ctx, [_job(ct, a, g, count=256, n_cols=3, global_base=i << 12)
                                          for i, a in enumerate(bufs)])
        assert lib.mh_ctx_kernel_time(gpu_ctx.h, C.byref(ms), C.byref(n)) == native.MH_OK
        assert n.value == 1 and 0.0 < ms.value < 1000.0, (n.value, ms.value)
    finally:
        lib.mh_ctx_enable_timing(gpu_ctx.h, 0)
        for a in bufs:
            a.close()
        ct.close()
