"""Spilled tapes on the device: the spill kernel variant (kernels.h kSpillVariant) and every launch
path that runs it, against the C oracle and the Python oracle.

A tape with more live values than the interpreter's 15 registers compiles with D_SPILL / D_FILL
(tests/test_spill_host.py checks the code on the host) and keeps the spilled values in device
memory, an area per wave.  Here: counts and first hits of such tapes in one-wave and 256-thread
workgroups, among tapes that do not spill, in values mode, in a batched round next to
mh_query_round, in an enumeration window, as conjunct masks of the repair step, in the C++ step()
library, and one query answered end to end.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import decide, native
from mythril_amd.tape import Op, TapeSet
from oracle import ctape
from oracle import smt_eval as E
from tests import batch_cases
from tests import spill_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, BASE = 0x5B111, 1000


def check_counts(ctx, ts, rows: int, row_first: int, want_spills) -> None:
    """mh_run in COUNT_ALL over rows [row_first, row_first + rows) of a generated buffer: counts
    and first hits equal the C oracle's; FIRST_HIT finds the same first hits."""
    ct = ctx.compile(ts)
    a = ctx.assignments(ts.n_vars, row_first + rows)
    try:
        want_spills(ct.spills())
        for i, inf in enumerate(ct.info()):
            if ct.spills()[i]:
                assert inf["n_regs"] == 15 and inf["features"] & 32 and inf["features"] & 8
            else:
                assert not inf["features"] & 32
        a.generate(SEED, BASE)
        cnt, first = ctape.count(ts, SEED, BASE + row_first, rows,
                                 threads=min(16, os.cpu_count() or 1))
        fh, hc = native.run(ctx, ct, a, row_first=row_first, row_count=rows, index_base=BASE,
                            mode=native.MODE_COUNT_ALL)
        assert np.array_equal(hc, cnt), (hc, cnt)
        assert np.array_equal(fh, first), (fh, first)
        assert int(np.count_nonzero(hc)) >= len(ts.tapes) // 2, "most tapes count some hits"
        fh1, _ = native.run(ctx, ct, a, row_first=row_first, row_count=rows, index_base=BASE,
                            mode=native.MODE_FIRST_HIT)
        assert np.array_equal(fh1, first)
    finally:
        a.close()
        ct.close()


def _want(n_cols, plain=False):
    fit = [t + (plain and t >= 8) for t in sc.MIXED_FIT[n_cols]] + ([8] if plain else [])

    def check(s):
        assert len(s) == 19 + plain and sorted(fit) == [t for t in range(len(s)) if s[t] == 0], s

    return check


# four columns: every column pinned; six and nine: every column a D_LOADVAR, which a spilled
# tape's kernel loads in its driver (the in-core LOADVAR is not safe across its re-entries)
@pytest.mark.parametrize("n_cols", [4, 6, 9])
def test_parity_one_wave_workgroups(gpu_ctx, n_cols):
    """209 rows from row 37: three waves and a partial one, each a workgroup of its own."""
    check_counts(gpu_ctx, sc.mixed_set(n_cols), 209, 37, _want(n_cols))


@pytest.mark.parametrize("n_cols", [4, 6])
def test_parity_256_thread_workgroups(gpu_ctx, n_cols):
    """4097 rows: the 256-thread workgroups (four waves share a workgroup's spill region)."""
    check_counts(gpu_ctx, sc.mixed_set(n_cols), 4097, 37, _want(n_cols))


@pytest.mark.parametrize("n_cols", [4, 6])
def test_mixed_set_splits_into_variants(gpu_ctx, n_cols):
    """The same set with a tape that does not spill in the middle: the launch splits into kernel
    variants and the results keep their tapes."""
    check_counts(gpu_ctx, sc.mixed_set(n_cols, plain=True), 209, 37, _want(n_cols, plain=True))


def test_sub_range_cuts_the_spill_bucket(gpu_ctx):
    """A run over tapes [tape_first, tape_first + tape_count) of the mixed set, both chosen from
    the set's spills() so that spilled and fitting tapes lie inside and outside the range: the
    spill variant's launch starts inside its bucket (a spill region for a part of the bucket's
    tapes), the results indexed from tape_first."""
    ts = sc.mixed_set(6, plain=True)
    rows, row_first = 209, 37
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(ts.n_vars, row_first + rows)
    try:
        s = [int(x) for x in ct.spills()]
        fit = [t for t in range(len(s)) if s[t] == 0]
        first, end = fit[0] + 1, fit[-1] + 2
        inside, outside = s[first:end], s[:first] + s[end:]
        assert 0 in inside and any(inside) and 0 in outside and any(outside), s
        a.generate(SEED, BASE)
        cnt, hit = ctape.count(ts, SEED, BASE + row_first, rows,
                               threads=min(16, os.cpu_count() or 1))
        for mode in (native.MODE_COUNT_ALL, native.MODE_FIRST_HIT):
            fh, hc = native.run(gpu_ctx, ct, a, tape_first=first, tape_count=end - first,
                                row_first=row_first, row_count=rows, index_base=BASE, mode=mode)
            assert np.array_equal(fh, hit[first:end]), (mode, fh, hit[first:end])
            if mode == native.MODE_COUNT_ALL:
                assert np.array_equal(hc, cnt[first:end]), (hc, cnt[first:end])
        assert np.count_nonzero(cnt[first:end]) >= (end - first) // 2, "most tapes count some hits"
    finally:
        a.close()
        ct.close()


def test_wide_fuzz_tapes(gpu_ctx):
    """150 fuzz tapes over six columns in one set (most spill), 128 rows: the sample on which
    spilled tapes over loaded columns once counted wrong in some lanes."""
    names = sc.MIXED_COLUMNS[:6]
    ts = TapeSet(names)
    b = ts.builder()
    for seed in range(150):
        _, n_ops, window = sc.fuzz_params(seed)
        ts.add(b.finish(sc.fuzz_into(b, names, seed, n_ops, window, mix=True)))
    check_counts(gpu_ctx, ts, 128, 0, lambda s: np.count_nonzero(s) > 100 or pytest.fail(str(s)))


def test_values_mode(gpu_ctx):
    """mh_eval_values of a spilled tape with a 256-bit root (the fan's t) over one row, and
    mh_eval_values_many / mh_eval_values_jobs of it next to a tape that fits."""
    ts = TapeSet(["x0", "x1"])
    b = ts.builder()
    ts.add(b.finish(sc.fan_nodes(b, 24, 2)[0]))
    ts.add(b.finish(sc.fan_nodes(b, 6, 1)[0]))
    ts.add(b.finish(sc.fan_nodes(b, 13, 1)[0]))
    rows = sc.edge_rows(2, 5, 7)
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(2, len(rows))
    try:
        assert [int(x > 0) for x in ct.spills()] == [1, 0, 1]
        a.upload(sc.soa(rows, 2))
        want = [[int(E.evaluate(t.nodes, ts.pool.values, r)) for r in rows] for t in ts.tapes]

        def word(limbs):
            return sum(int(limbs[k]) << (32 * k) for k in range(8))

        for r in range(len(rows)):
            got = native.eval_values(gpu_ctx, ct, 0, a, r, 1)
            assert word(got[:, 0]) == want[0][r], r
        many = native.eval_values_many(gpu_ctx, ct, [2, 1, 0, 2], a, 3)
        assert [word(many[i]) for i in range(4)] == [want[2][3], want[1][3], want[0][3], want[2][3]]
        jobs = native.eval_values_jobs(gpu_ctx, [(ct, None, [0, 1, 2], a, 2),
                                                 (ct, None, [2], a, 4)])
        assert [word(jobs[0][i]) for i in range(3)] == [want[t][2] for t in range(3)]
        assert word(jobs[1][0]) == want[2][4]
    finally:
        a.close()
        ct.close()


def test_values_mode_two_waves(gpu_ctx):
    """mh_eval_values of the spilled fan tape above over 65 rows: two waves, the smallest run
    with more than one wave's spill area; every row's value against the Python oracle."""
    ts = TapeSet(["x0", "x1"])
    b = ts.builder()
    ts.add(b.finish(sc.fan_nodes(b, 24, 2)[0]))
    rows = sc.edge_rows(2, 65, 7)
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(2, len(rows))
    try:
        assert ct.spills()[0] > 0
        a.upload(sc.soa(rows, 2))
        got = native.eval_values(gpu_ctx, ct, 0, a, 0, len(rows))
        assert got.shape == (8, 65)
        for r, row in enumerate(rows):
            want = int(E.evaluate(ts.tapes[0].nodes, ts.pool.values, row))
            assert sum(int(got[k, r]) << (32 * k) for k in range(8)) == want, r
    finally:
        a.close()
        ct.close()


def test_batched_round_equals_single_rounds(gpu_ctx):
    """mh_query_round_many with three jobs -- spilling with one slot, spilling with many, not
    spilling -- equals three mh_query_round calls: the spilling jobs share one launch, whose
    waves take disjoint areas of one region."""
    g = batch_cases.HostGuide(batch_cases.flat_guide(2))
    sets = [("one_slot", sc.fan(13), 200, 1), ("many_slots", sc.fan(40), 64, 28),
            ("fits", sc.fan(10), 130, 0)]
    jobs, handles = [], []
    try:
        for i, (name, ts, count, slots) in enumerate(sets):
            ct = gpu_ctx.compile(ts)
            a = gpu_ctx.assignments(2, 256)
            handles += [ct, a]
            assert int(ct.spills()[0]) == slots
            jobs.append(dict(name=name, tapes=ct, assign=a, guide=g, seed=11 + i,
                             global_base=500 * i, count=count, n_cols=2,
                             mode=native.MODE_COUNT_ALL))
        want = batch_cases.run_sequential(gpu_ctx, jobs)
        got = batch_cases.run_batched(gpu_ctx, jobs)
        assert batch_cases.assert_equal(jobs, want, got) == 3
        # and the counts are the oracle's, not only equal to each other
        for j, w in zip(jobs, want):
            ts = next(s[1] for s in sets if s[0] == j["name"])
            rows = w[3]
            hits = [r for r in range(j["count"]) if E.evaluate(
                ts.tapes[0].nodes, ts.pool.values,
                [sum(int(rows[c, k, r]) << (32 * k) for k in range(8)) for c in range(2)])]
            assert int(w[1][0]) == len(hits) and int(w[0][0]) == j["global_base"] + hits[0]
    finally:
        for h in handles:
            h.close()


def test_enumeration_window(gpu_ctx):
    """One mh_query_enumerate window over a spilled tape with two 16-value domain columns,
    against brute force over the 256 rows."""
    ts = sc.fan(16, 2)
    rng = random.Random(5)
    lo = (1 << 255) - 8
    vals = sorted(rng.getrandbits(256) for _ in range(16))
    d = native.domains_create(cols=[0, 1], kinds=[native.DOMAIN_INTERVAL, native.DOMAIN_LIST],
                              sizes=[16, 16], los=[lo, 0], lists=[[], vals], widths=[256, 256])
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(2, 256)
    try:
        assert ct.spills()[0] > 0
        rows = decide.enumerate_rows(d, 0, 256)
        hits = [r for r, row in enumerate(rows)
                if E.evaluate(ts.tapes[0].nodes, ts.pool.values, row)]
        assert 16 < len(hits) < 240
        fh, hc, out = native.query_enumerate(gpu_ctx, ct, a, d, 0, 256, 2,
                                             mode=native.MODE_COUNT_ALL)
        assert int(hc[0]) == len(hits) and int(fh[0]) == hits[0]
        got = [sum(int(out[0, c, k]) << (32 * k) for k in range(8)) for c in range(2)]
        assert got == rows[hits[0]]
    finally:
        a.close()
        ct.close()
        d.close()


def test_repair_score_masks(gpu_ctx):
    """mh_repair_score over four conjunct tapes of which one spills: the masks-mode launch of
    the spill variant; per-row fail counts equal the oracle's."""
    ts = TapeSet(["x0", "x1"])
    b = ts.builder()
    x0, x1 = b.var("x0", 256), b.var("x1", 256)
    ts.add(b.finish(b.op(Op.BVULT, x0, b.const(1 << 255, 256))))
    ts.add(b.finish(sc.fan_nodes(b, 24, 1)[1]))
    ts.add(b.finish(b.op(Op.BVUGT, b.op(Op.BVADD, x0, x1), b.const(1 << 254, 256))))
    ts.add(b.finish(b.op(Op.EQ, b.op(Op.BVAND, x1, b.const(3, 256)), b.const(1, 256))))
    n = 300
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(2, n)
    rep = native.repair_open(gpu_ctx, 4, 512, 8)
    try:
        assert [int(x > 0) for x in ct.spills()] == [0, 1, 0, 0]
        a.generate(SEED, BASE)
        fails = native.repair_score(rep, ct, a, counts=True)
        want = []
        for r in range(n):
            row = E.gen_assignment(SEED, 2, BASE + r)
            want.append(sum(0 if E.evaluate(t.nodes, ts.pool.values, row) else 1
                            for t in ts.tapes))
        assert [int(x) for x in fails] == want
    finally:
        rep.close()
        a.close()
        ct.close()


def test_sieve_answers_a_query_that_spills(gpu_ctx):
    """Sieve.solve on ULT(t, 2^255) over the fan k = 13: refused for register pressure before the
    interpreter could spill; now a witness the oracle accepts, and one spilled tape counted."""
    from mythril_amd import smt
    from mythril_amd.sieve import Sieve

    qctx = smt.Context()
    smt.set_context(qctx)
    b = qctx.b
    t, _ = sc.fan_nodes(b, 13, 1, var=b.user_var)
    root = b.op(Op.BVULT, t, b.const(1 << 255, 256))
    s = Sieve()
    try:
        w = s.solve(b, [root])
        assert w is not None, "no witness"
        assert s.stats.extra.get("spilled_tapes") == 1, s.stats.extra
        assert not s.stats.extra.get("sieve_unsupported")
    finally:
        s.close()
    names = [n for n, _ in sorted(b.var_index.items(), key=lambda kv: kv[1])]
    row = [int(w.values.get(n, 0)) for n in names]
    assert E.evaluate(b.finish(root).nodes, b.pool.values, row)


def test_cpp_step_library(gpu_ctx):
    """The first parity case in the MH_ASM_CORE=0 library (D_SPILL / D_FILL through exec.h's
    step()), in a child process with MYTHRIL_HIP_LIB naming it."""
    lib = os.path.join(ROOT, "mythril_amd", "libmythril_hip_noasm.so")
    assert os.path.exists(lib), "build it first: make -C mythril_amd/csrc noasm (build() does)"
    r = subprocess.run([sys.executable, "-u", "-m", "tests.noasm_spill_check"], cwd=ROOT,
                       env=dict(os.environ, MYTHRIL_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "noasm spill ok: 19 + 19 tapes" in r.stdout
