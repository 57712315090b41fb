"""mh_run / mh_run_async over row windows, tape ranges and accumulated result buffers, against the
C oracle (tests/partition_cases.py has the inputs; tests/test_partition_cases.py checks them on
the host).  Every comparison is exact equality of u64 with ``ctape.count`` of the same rows.

Three engines run the same tape sets over one generated buffer of N rows:

``interp``  the interpreter (one-wave workgroups up to 4096 rows, 256-thread ones above; merged
            launches for a short run over the whole set);
``split``   compiled under MH_SPLIT_INSNS=8: runs of up to 65536 rows walk the conjunct parts in
            masks mode and the combine kernel ANDs them, longer runs walk whole tapes;
``jit``     after ``ct.jit()``: a whole-set run goes through the native code (and the interpreter
            for what it refused), a tape sub-range through the interpreter alone.

In FIRST_HIT mode only first_hit is compared (hit_count is not a function of the arguments there).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import native
from tests import partition_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = ("interp", "split", "jit")
MODES = {"count_all": native.MODE_COUNT_ALL, "first_hit": native.MODE_FIRST_HIT}
BASE, N = pc.BASE, pc.N


def compile_engine(ctx, name, engine):
    """The set compiled for `engine`, with what makes it that engine asserted."""
    ts = pc.tape_set(name)
    old = os.environ.get("MH_SPLIT_INSNS")
    try:
        os.environ["MH_SPLIT_INSNS"] = "8" if engine == "split" else "0"
        ct = ctx.compile(ts)
    finally:
        if old is None:
            os.environ.pop("MH_SPLIT_INSNS", None)
        else:
            os.environ["MH_SPLIT_INSNS"] = old
    n_split, n_parts, parts = ct.split_info()
    if engine == "split":
        conj = pc.planted_conjunctions(name)
        assert n_split >= len(conj) and n_parts >= 2 * n_split, (n_split, n_parts)
        assert all(parts[t] >= 2 for t in conj), ("planted conjunctions not split", parts)
        assert n_split == np.count_nonzero(parts) and n_parts == int(parts.sum())
    else:
        assert (n_split, n_parts) == (0, 0) and not parts.any()
    if engine == "jit":
        info = ct.jit()
        jitted = ct.jitted()
        assert all(jitted[t] for t in pc.planted(name) + pc.planted_conjunctions(name)), jitted
        assert info["n_jitted"] == int(jitted.sum())
    if name == "spill":
        s = ct.spills()
        assert s[0] > 0 and s[1] == 0 and np.count_nonzero(s[:pc.SPILL_HEAD]) >= 3, s
    return ct


class Rig:
    """Per tape set: the generated buffer and the compiled engines, made on first use."""

    def __init__(self, ctx):
        self.ctx, self.bufs, self.cts = ctx, {}, {}

    def buf(self, name):
        if name not in self.bufs:
            a = self.ctx.assignments(pc.tape_set(name).n_vars, N)
            a.generate(pc.SEED, BASE)
            self.bufs[name] = a
        return self.bufs[name]

    def ct(self, name, engine):
        if (name, engine) not in self.cts:
            self.cts[name, engine] = compile_engine(self.ctx, name, engine)
        return self.cts[name, engine]

    def close(self):
        for h in list(self.cts.values()) + list(self.bufs.values()):
            h.close()


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    r = Rig(gpu_ctx)
    yield r
    r.close()


def differing(got, want):
    return [(t, int(got[t]), int(want[t])) for t in range(len(want)) if int(got[t]) != int(want[t])]


def check(fh, hc, cnt, hit, mode, where):
    """(first_hit, hit_count) of a run against the oracle's (cnt, hit) of the same rows."""
    assert fh.dtype == np.uint64 and hc.dtype == np.uint64
    assert np.array_equal(fh, hit), (where, "first_hit", differing(fh, hit))
    if mode == native.MODE_COUNT_ALL:
        assert np.array_equal(hc, cnt), (where, "hit_count", differing(hc, cnt))
    for t in np.flatnonzero(cnt == 0):  # said once more, in the test's own words
        assert int(fh[t]) == native.NO_HIT, (where, int(t))
        if mode == native.MODE_COUNT_ALL:
            assert int(hc[t]) == 0, (where, int(t))


@pytest.mark.parametrize("window", pc.WINDOWS, ids=lambda w: "%d+%d" % w)
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_windows(rig, name, engine, window):
    """One run over rows [first, first + count) of the buffer, both modes."""
    first, count = window
    cnt, hit = pc.oracle(name, first, count)
    ct, a = rig.ct(name, engine), rig.buf(name)
    for mname, mode in MODES.items():
        fh, hc = native.run(rig.ctx, ct, a, row_first=first, row_count=count, index_base=BASE,
                            mode=mode)
        check(fh, hc, cnt, hit, mode, (name, engine, window, mname))


@pytest.mark.parametrize("partition", ("whole", "ends", "cut_conjunctions"))
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_tape_ranges(rig, name, engine, partition):
    """Runs over tapes [tape_first, tape_first + tape_count): results indexed from tape_first equal
    the oracle's slice.  A sub-range of a jitted set is the interpreter's; the cut through the
    planted conjunctions runs a part of the split tapes' parts and combines only those."""
    ct, a = rig.ct(name, engine), rig.buf(name)
    for first, count in pc.RANGE_WINDOWS:
        cnt, hit = pc.oracle(name, first, count)
        for tf, tc in pc.tape_partitions(name)[partition]:
            for mname, mode in MODES.items():
                fh, hc = native.run(rig.ctx, ct, a, tape_first=tf, tape_count=tc, row_first=first,
                                    row_count=count, index_base=BASE, mode=mode)
                assert len(fh) == tc and len(hc) == tc
                check(fh, hc, cnt[tf:tf + tc], hit[tf:tf + tc], mode,
                      (name, engine, (first, count), (tf, tc), mname))


# ---- accumulation: mh_run_async does not reset its result buffers --------------------------------
def device_results(n, first_hit=None, hit_count=None):
    """Two int64 device tensors of n; a value given pre-seeds every entry (and then nothing resets
    the buffer), None leaves it to mh_results_reset."""
    import torch

    fh = torch.empty(n, dtype=torch.int64, device="cuda")
    hc = torch.empty(n, dtype=torch.int64, device="cuda")
    if first_hit is not None:
        fh.fill_(first_hit if first_hit < 1 << 63 else first_hit - (1 << 64))
        hc.fill_(hit_count)
        torch.cuda.synchronize()  # the fills ran on torch's stream, the runs use the context's
    return fh, hc


def accumulate(rig, ct, a, n, calls, mode, seed=None):
    """One reset (or the pre-seeded values `seed` = (first_hit, hit_count)), then every call
    (row_first, row_count, tape_first, tape_count) with mh_run_async into the same buffers, the
    pointers offset by tape_first; one synchronize at the end.  Returns (first_hit, hit_count)."""
    fh, hc = device_results(n, *(seed or (None, None)))
    if seed is None:
        native.results_reset(rig.ctx, fh.data_ptr(), hc.data_ptr(), n)
    for first, count, tf, tc in calls:
        native.run_async(rig.ctx, ct, a, fh.data_ptr() + 8 * tf, hc.data_ptr() + 8 * tf,
                         tape_first=tf, tape_count=tc, row_first=first, row_count=count,
                         index_base=BASE, mode=mode)
    rig.ctx.synchronize()
    return fh.cpu().numpy().view(np.uint64), hc.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("tiling", sorted(pc.TILINGS))
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_accumulated_row_tilings(rig, name, engine, tiling):
    """The buffer run piece by piece into one pair of result buffers, reset once: SUM of counts
    and MIN of first hits, whatever the order.  Ascending, a FIRST_HIT launch meets the minimum the
    earlier ones left and may skip; descending, each launch's atomic MIN has to lower it."""
    ct, a = rig.ct(name, engine), rig.buf(name)
    n = ct.n_tapes
    cnt, hit = pc.oracle(name, 0, N)
    for oname, order in pc.orders(pc.TILINGS[tiling]).items():
        calls = [(f, c, 0, n) for f, c in order]
        for mname, mode in MODES.items():
            fh, hc = accumulate(rig, ct, a, n, calls, mode)
            check(fh, hc, cnt, hit, mode, (name, engine, tiling, oname, mname))


@pytest.mark.parametrize("partition", ("ends", "cut_conjunctions"))
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_accumulated_rows_and_tape_ranges(rig, name, engine, partition):
    """Row tiling x tape-range partition: every (window, range) cell runs once, each call's
    buffers offset by its tape_first."""
    ct, a = rig.ct(name, engine), rig.buf(name)
    cnt, hit = pc.oracle(name, 0, N)
    ranges = pc.tape_partitions(name)[partition]
    calls = [(f, c, tf, tc) for f, c in pc.orders(pc.TILE_A)["shuffled"] for tf, tc in ranges]
    for mname, mode in MODES.items():
        fh, hc = accumulate(rig, ct, a, ct.n_tapes, calls, mode)
        check(fh, hc, cnt, hit, mode, (name, engine, partition, mname))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", pc.SET_NAMES)
def test_preseeded_buffers(rig, name, engine):
    """Buffers that hold earlier results and are not reset: a first hit below every index of the
    run survives both modes, a count is added to, a first hit inside the run is lowered only by
    the tapes that hit before it."""
    ct, a = rig.ct(name, engine), rig.buf(name)
    n = ct.n_tapes
    cnt, hit = pc.oracle(name, 0, N)
    calls = [(f, c, 0, n) for f, c in pc.TILE_A]
    for mname, mode in MODES.items():
        where = (name, engine, mname)
        fh, hc = accumulate(rig, ct, a, n, calls, mode, seed=(BASE - 1, 0))
        assert (fh == np.uint64(BASE - 1)).all(), (where, "earlier minimum", differing(
            fh, np.full(n, BASE - 1, dtype=np.uint64)))
        if mode == native.MODE_COUNT_ALL:
            assert np.array_equal(hc, cnt), (where, differing(hc, cnt))
        fh, hc = accumulate(rig, ct, a, n, calls, mode, seed=(native.NO_HIT, 1000))
        assert np.array_equal(fh, hit), (where, "after NO_HIT", differing(fh, hit))
        if mode == native.MODE_COUNT_ALL:
            want = cnt + np.uint64(1000)
            assert np.array_equal(hc, want), (where, "1000 + count", differing(hc, want))
        mid = BASE + 4133
        fh, hc = accumulate(rig, ct, a, n, calls, mode, seed=(mid, 0))
        want = np.minimum(hit, np.uint64(mid))
        assert np.array_equal(fh, want), (where, "minimum inside the run", differing(fh, want))
        assert (want == np.uint64(mid)).any() and (want < np.uint64(mid)).any()
        if mode == native.MODE_COUNT_ALL:
            assert np.array_equal(hc, cnt), (where, differing(hc, cnt))


# ---- the native kernel with several 64-row chunks per wave ---------------------------------------
@pytest.mark.parametrize("rows_per_wg", [512, 1024])
def test_jit_chunk_loop_forced(gpu_ctx, rows_per_wg):
    """MH_JIT_ROWS_PER_WG (read once per process) makes each wave of the native kernel walk 2 or 4
    chunks; short windows then end in a partial chunk, in a chunk clipped away, or before a
    workgroup's later waves begin.  tests/jit_rows_check.py compares both modes with the C oracle
    in a child process of its own."""
    env = dict(os.environ, MH_JIT_ROWS_PER_WG=str(rows_per_wg))
    r = subprocess.run([sys.executable, "-u", "-m", "tests.jit_rows_check"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("jit rows ok: %d rows per workgroup" % rows_per_wg), last


def test_jit_two_chunks_per_wave_by_size(gpu_ctx):
    """2^19 + 77 rows: the smallest run whose workgroups take 512 rows on their own (capi.cpp
    jit_rows_per_wg), so each wave walks two chunks and the last workgroup ends 77 rows in --
    planted rows on both sides of row 2^19 and on the last row, from an aligned and an unaligned
    start."""
    assert "MH_JIT_ROWS_PER_WG" not in os.environ
    ts = pc.tape_set("big")
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(ts.n_vars, pc.BIG_N)
    try:
        ct.jit()
        jitted = ct.jitted()
        assert all(jitted[t] for t in pc.planted("big") + pc.planted_conjunctions("big")), jitted
        a.generate(pc.SEED, BASE)
        for first, count in ((0, pc.BIG_N), (37, pc.BIG_N - 37)):
            assert count > 1 << 19
            cnt, hit = pc.oracle("big", first, count)
            for t, m in zip(pc.planted("big"), pc.BIG_MARKS):
                assert int(cnt[t]) == int(m >= first), "the marks are the oracle's"
            for mname, mode in MODES.items():
                fh, hc = native.run(gpu_ctx, ct, a, row_first=first, row_count=count,
                                    index_base=BASE, mode=mode)
                check(fh, hc, cnt, hit, mode, ("big", "jit", (first, count), mname))
    finally:
        a.close()
        ct.close()
