"""mh_eval_values_jobs and mh_tables_create_many on the device: every job of a submission equals,
bit for bit, the single call it stands for (mh_eval_values_tables at one row, mh_eval_values_many
without tables), on the tapes of tests/lookup_cases.py and table-free ones.  One call mixing all
three register classes, table and table-free variants, a keccak and a complex-op tape, keys of 1,
2 and 3 words and an empty table; a job of one tape and one of 65 tapes that a single workgroup
walks (across the 64-tape chunk); repeated and descending ids; 8 jobs sharing one buffer with
different column meanings; 256 jobs accepted, 257 refused; every refusal leaves `out` as it was
and launches nothing; the C++ step() library; table sets made in one allocation.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import native
from mythril_amd.tape import Op, TapeSet
from tests import fake_tables, lookup_cases, values_jobs_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5A5A5A5


@pytest.fixture
def handles(gpu_ctx):
    h = cases.Handles(gpu_ctx, native)
    yield h
    h.close()


def test_mixed_jobs_equal_single_calls(gpu_ctx, handles):
    jobs, seen = cases.mixed_jobs(handles)
    # every register class with and without a table: six of the variants at least, one launch each
    assert seen >= {(c, t) for c in range(3) for t in (False, True)}, seen
    before = native.eval_launches(gpu_ctx)
    got = native.eval_values_jobs(gpu_ctx, jobs)
    launches = native.eval_launches(gpu_ctx) - before
    assert 6 <= launches <= 15, launches  # one per variant present, never one per job
    for i, job in enumerate(jobs):
        want = cases.single(gpu_ctx, native, job)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), i


def test_jobs_share_one_buffer_with_different_columns(gpu_ctx, handles):
    """8 jobs at rows 0..7 of one 3-column buffer: row r holds a key of 1 + r % 3 words for a
    tape set over that many columns, so column 1 means another thing in every job."""
    rng = lookup_cases.case_rng(9100)
    sets, keys, nws = {}, [], []
    for nw in (1, 2, 3):
        table, els = lookup_cases.make_table(rng, 64, nw, 256)
        sets[nw] = (handles.compile(lookup_cases.lookup_tapeset(nw, 256)),
                    handles.tables([(table, els, 256 * nw)]), table, els)
    for r in range(8):
        nw = 1 + r % 3
        table = sets[nw][2]
        keys.append(sorted(table)[r] if r % 2 == 0 else rng.getrandbits(256 * nw))
        nws.append(nw)
    a = handles.assign(3, keys, nws)
    jobs = [(sets[nws[r]][0], sets[nws[r]][1], [0, 1], a, r) for r in range(8)]
    got = cases.check_jobs(gpu_ctx, native, jobs)
    for r in range(8):
        _, _, table, els = sets[nws[r]]
        vals = native.limbs_to_ints(got[r].T)
        assert vals == [fake_tables.lookup_ref(table, els, keys[r]),
                        fake_tables.lookup_ref(table, els, keys[r], hit=True)], r


def many_tapes(n):
    ts = TapeSet()
    b = ts.builder()
    x = b.var("k0", 256)
    for i in range(n):
        ts.add(b.finish(b.op(Op.BVXOR, b.op(Op.BVADD, x, b.const(i * i + 1, 256)), x)))
    return ts


def test_256_jobs_and_a_65_tape_job(gpu_ctx, handles):
    """256 jobs of one variant are one launch of 256 workgroups, none split: the job of 65 tapes
    is walked by one workgroup across the 64-tape chunk.  Alone, the same job is split a
    workgroup per tape.  Both equal the single call."""
    ct = handles.compile(many_tapes(70))
    rows = [0x1234567 * (r + 1) << (r % 200) for r in range(256)]
    a = handles.assign(1, rows)
    long_ids = list(range(69, 4, -1))
    assert len(long_ids) == 65
    jobs = [(ct, None, long_ids if r == 7 else [r % 70], a, r) for r in range(256)]
    before = native.eval_launches(gpu_ctx)
    cases.check_jobs(gpu_ctx, native, jobs)
    # the batch's one launch, then one per single call of the comparison
    assert native.eval_launches(gpu_ctx) - before == 1 + 256
    cases.check_jobs(gpu_ctx, native, [jobs[7]])
    cases.check_jobs(gpu_ctx, native, [(ct, None, [3], a, 255)])


def raw_call(ctx, specs):
    """mh_eval_values_jobs on (ts handle, tables handle, ids, assign handle, row) with every `out`
    prefilled: (code, message, outs)."""
    arr = (native.ValuesJob * max(len(specs), 1))()
    keep = []
    for k, (ts, tb, ids, a, row) in enumerate(specs):
        ids_a = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.full((max(len(ids_a), 1), 8), SENTINEL, dtype=np.uint32)
        arr[k] = native.ValuesJob(ts, tb, native._ptr(ids_a) if len(ids_a) else None, len(ids_a),
                                  a, row, native._ptr(out))
        keep.append((ids_a, out))
    r = ctx.lib.mh_eval_values_jobs(ctx.h, arr, len(specs))
    return r, ctx.lib.mh_last_error().decode(), [o for _, o in keep]


def test_refusals_touch_nothing(gpu_ctx, handles):
    ct = handles.compile(lookup_cases.lookup_tapeset(1, 256))
    plain = handles.compile(cases.plain_tapeset())
    a = handles.assign(1, [5, 6])
    tb = handles.tables([({5: 9}, 1, 256)])
    good = [(ct.h, tb.h, [0, 1, 2], a.h, 0), (plain.h, None, [0, 1], a.h, 1)]
    r, _, outs = raw_call(gpu_ctx, good)
    assert r == native.MH_OK and all((o != SENTINEL).any() for o in outs)
    other = native.Context(0)
    try:
        foreign = cases.Handles(other, native)
        f_ct = foreign.compile(cases.plain_tapeset())
        f_tb = foreign.tables([({5: 9}, 1, 256)])
        f_a = foreign.assign(1, [5])
        no_table = handles.tables([])
        wide_key = handles.tables([({}, 0, 512)])
        bad = {
            "null tape set": ((None, None, [0], a.h, 0), native.MH_E_INVALID, "null"),
            "null buffer": ((plain.h, None, [0], None, 0), native.MH_E_INVALID, "null"),
            "foreign tape set": ((f_ct.h, None, [0], a.h, 0), native.MH_E_INVALID, "another ctx"),
            "foreign buffer": ((plain.h, None, [0], f_a.h, 0), native.MH_E_INVALID, "another ctx"),
            "foreign tables": ((ct.h, f_tb.h, [0], a.h, 0), native.MH_E_INVALID, "another ctx"),
            "row out of bounds": ((plain.h, None, [0], a.h, 2), native.MH_E_INVALID, "row"),
            "tape id out of bounds": ((plain.h, None, [0, 99], a.h, 0), native.MH_E_INVALID,
                                      "tape id"),
            "table the set lacks": ((ct.h, no_table.h, [0], a.h, 0), native.MH_E_INVALID,
                                    "names table"),
            "key words differ": ((ct.h, wide_key.h, [0], a.h, 0), native.MH_E_INVALID, "words"),
            "lookup without tables": ((ct.h, None, [1], a.h, 0), native.MH_E_UNSUPPORTED,
                                      "lookup"),
        }
        before = native.eval_launches(gpu_ctx)
        for what, (spec, code, word) in bad.items():
            r, msg, outs = raw_call(gpu_ctx, good + [spec])
            assert r == code and "job 2" in msg and word in msg, (what, r, msg)
            assert all((o == SENTINEL).all() for o in outs), what
        # 257 jobs, each valid
        r, msg, outs = raw_call(gpu_ctx, [good[1]] * 257)
        assert r == native.MH_E_INVALID and "MH_VALUES_JOBS_MAX" in msg
        assert all((o == SENTINEL).all() for o in outs)
        assert native.eval_launches(gpu_ctx) == before  # nothing was launched
        assert raw_call(gpu_ctx, [])[0] == native.MH_OK
        foreign.close()
    finally:
        other.close()


def test_refuses_a_variant_the_capacity_does_not_fit(gpu_ctx, handles):
    """A buffer of 2^30 + 64 rows per column: a keccak tape (32-bit limb-plane stride) is
    refused for the whole list, an asm-only one runs at the buffer's last row."""
    cap = (1 << 30) + 64
    plain = handles.compile(cases.plain_tapeset())
    n = len(cases.plain_tapeset().tapes)
    big = gpu_ctx.assignments(1, cap)
    handles.open.append(big)
    soa = lookup_cases.key_soa([0xABCDEF << 77], 1)
    big.upload(soa, first=cap - 1)
    before = native.eval_launches(gpu_ctx)
    r, msg, outs = raw_call(gpu_ctx, [(plain.h, None, [0], big.h, cap - 1),
                                      (plain.h, None, [n - 2], big.h, cap - 1)])
    assert r == native.MH_E_UNSUPPORTED and "job 1" in msg and "2^30 rows" in msg, (r, msg)
    assert all((o == SENTINEL).all() for o in outs)
    assert native.eval_launches(gpu_ctx) == before
    cases.check_jobs(gpu_ctx, native, [(plain, None, [0, 1], big, cap - 1)])


def test_cpp_step_library(gpu_ctx):
    """The MH_ASM_CORE=0 library has the batched table kernels too (one child process with
    MYTHRIL_HIP_LIB naming it: tests/noasm_values_jobs_check.py)."""
    lib = os.path.join(ROOT, "mythril_amd", "libmythril_hip_noasm.so")
    assert os.path.exists(lib), "build it first: make -C mythril_amd/csrc noasm (build() does)"
    r = subprocess.run([sys.executable, "-u", "-m", "tests.noasm_values_jobs_check"], cwd=ROOT,
                       env=dict(os.environ, MYTHRIL_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "noasm values jobs ok" in r.stdout


def table_sets():
    rng = lookup_cases.case_rng(9200)
    sets = []
    for nw, n in ((1, 65), (2, 3), (3, 64)):
        t0, e0 = lookup_cases.make_table(rng, n, nw, 256)
        sets.append([(t0, e0, 256 * nw), ({}, 11 * nw, 256 * nw)])
    sets.insert(2, [])  # a set without tables
    return sets


def test_tables_create_many_reads_like_single_sets(gpu_ctx, handles):
    sets = table_sets()
    many = native.tables_create_many(gpu_ctx, sets)
    handles.open.extend(many)
    assert len(many) == len(sets)
    probes = {}
    jobs_many, jobs_single = [], []
    for s, tabs in enumerate(sets):
        if not tabs:
            continue
        nw = tabs[0][2] // 256
        keys = sorted(tabs[0][0])[:3] + [1, (1 << (256 * nw)) - 1]
        probes[s] = keys
        a = handles.assign(nw, keys)
        one = handles.tables(tabs)
        for tid in range(2):
            ct = handles.compile(lookup_cases.lookup_tapeset(nw, 256, table=tid))
            for r in range(len(keys)):
                jobs_many.append((ct, many[s], [0, 1], a, r))
                jobs_single.append((ct, one, [0, 1], a, r))
    got = cases.check_jobs(gpu_ctx, native, jobs_many)
    want = native.eval_values_jobs(gpu_ctx, jobs_single)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # destroying all but one leaves that one usable (the block lives until the last handle)
    keep = 3
    for s, tb in enumerate(many):
        if s != keep:
            tb.close()
    left = [(j, w) for j, w in zip(jobs_many, want) if j[1] is many[keep]]
    assert left
    again = native.eval_values_jobs(gpu_ctx, [j for j, _ in left])
    assert all(np.array_equal(g, w) for g, (_, w) in zip(again, left))


def test_tables_create_many_one_unsorted_set_creates_none(gpu_ctx):
    sets = table_sets()
    flat = [t for s in sets for t in s]
    counts, nws, koffs, keys, voffs, vals, elses, n_keys, n_vals = native.pack_tables(flat)
    per_set = np.ascontiguousarray([len(s) for s in sets], dtype=np.uint32)
    p = native._ptr

    def create(keys):
        hs = (C.c_void_p * len(sets))(*([1] * len(sets)))
        r = gpu_ctx.lib.mh_tables_create_many(gpu_ctx.h, len(sets), p(per_set), p(counts), p(nws),
                                              p(koffs, C.c_uint64), p(keys), n_keys,
                                              p(voffs, C.c_uint64), p(vals), n_vals, p(elses), hs)
        return r, gpu_ctx.lib.mh_last_error().decode(), list(hs)

    r, _, hs = create(keys)
    assert r == native.MH_OK and all(hs)
    for h in hs:
        gpu_ctx.lib.mh_tables_destroy(C.c_void_p(h))
    bad = keys.copy()
    at = int(koffs[2])  # set 1's first table: swap its first two entries' low limbs' order
    k0, k1 = bad[at:at + 16].copy(), bad[at + 16:at + 32].copy()
    bad[at:at + 16], bad[at + 16:at + 32] = k1, k0
    r, msg, hs = create(bad)
    assert r == native.MH_E_INVALID and "set 1" in msg and "ascending" in msg, (r, msg)
    assert not any(hs)  # nothing created: every handle cleared
