"""D_LOOKUP on the device (the F_TABLE kernel variants, mh_tables_create, mh_eval_values_tables)
against the Python restatement tests/fake_tables.lookup_ref, on the table shapes of
tests/lookup_cases.py: tables of 0, 1, 2, 3, 64 and 65 entries, keys of 1, 2 and 3 words that
differ only in limb 0 or only in the top limb of the top word, probes at and around every edge,
range widths 8, 160 and 256, the value and the hit form; row counts around the wave size with a
different key per row; every register class; the C++ step() library; tapes that mix the lookup
with KECCAK and with a division; and the refusals.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import native
from oracle import smt_eval
from tests import fake_tables, lookup_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nw", [1, 2, 3])
def test_table_shapes(gpu_ctx, nw):
    assert lookup_cases.check_shapes(gpu_ctx, native, nws=(nw,)) == 6 * 3 * 2 * 65


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_row_counts(gpu_ctx, rows):
    """A different key per row: the lanes' searches diverge."""
    nw, width = 2, 256
    rng = lookup_cases.case_rng(rows, 77)
    table, els = lookup_cases.make_table(rng, 65, nw, width)
    keys = lookup_cases.probes(rng, table, nw, rows)
    assert len(set(keys)) == rows
    got, _ = lookup_cases.device_values(gpu_ctx, lookup_cases.lookup_tapeset(nw, width), [0, 1],
                                        [(table, els, 256 * nw)],
                                        lookup_cases.key_soa(keys, nw), native)
    assert got[0] == [fake_tables.lookup_ref(table, els, k) for k in keys]
    assert got[1] == [fake_tables.lookup_ref(table, els, k, hit=True) for k in keys]


@pytest.mark.parametrize("live,nr", [(0, 7), (6, 9), (10, 15)])
def test_register_classes(gpu_ctx, live, nr):
    """The lookup among `live` values held in registers: the NR 7, 9 and 15 table kernels."""
    nw, width = 2, 160
    rng = lookup_cases.case_rng(live, 78)
    table, els = lookup_cases.make_table(rng, 64, nw, width)
    keys = lookup_cases.probes(rng, table, nw, 65)
    ts = lookup_cases.lookup_tapeset(nw, width, live=live)
    tabs = [(table, els, 256 * nw)]
    got, info = lookup_cases.device_values(gpu_ctx, ts, [2], tabs,
                                           lookup_cases.key_soa(keys, nw), native)
    n_regs = int(info[2]["n_regs"])
    assert {7: n_regs <= 7, 9: 7 < n_regs <= 9, 15: 9 < n_regs <= 15}[nr], n_regs
    assert int(info[2]["features"]) & 16  # F_TABLE
    extra = fake_tables.lookup_extra(tabs)
    want = [int(smt_eval.evaluate(ts.tapes[2].nodes, ts.pool.values,
                                  [k & ((1 << 256) - 1), k >> 256], extra=extra)) for k in keys]
    assert got[0] == want


def test_lookup_mixed_with_keccak_and_division(gpu_ctx):
    rng = lookup_cases.case_rng(79)
    table, els = lookup_cases.make_table(rng, 65, 1, 256)
    keys = lookup_cases.probes(rng, table, 1, 65)
    ts = lookup_cases.mixed_tapeset()
    tabs = [(table, els, 256)]
    got, info = lookup_cases.device_values(gpu_ctx, ts, [0, 1], tabs,
                                           lookup_cases.key_soa(keys, 1), native)
    assert int(info[0]["features"]) & 2 and int(info[1]["features"]) & 1  # keccak, division
    extra = fake_tables.lookup_extra(tabs)
    for i in range(2):
        want = [int(smt_eval.evaluate(ts.tapes[i].nodes, ts.pool.values, [k], extra=extra))
                for k in keys]
        assert got[i] == want, i
    assert any(k in table for k in keys) and any(k not in table for k in keys)


def test_several_tables_in_one_set(gpu_ctx):
    """Table ids select their table; an empty table in the middle of the set is legal."""
    rng = lookup_cases.case_rng(80)
    t0, e0 = lookup_cases.make_table(rng, 3, 1, 256)
    t2, e2 = lookup_cases.make_table(rng, 64, 1, 256)
    tabs = [(t0, e0, 256), ({}, 7, 256), (t2, e2, 256)]
    keys = sorted(t0) + sorted(t2)[:5] + [1, 2]
    for tid in range(3):
        got, _ = lookup_cases.device_values(gpu_ctx, lookup_cases.lookup_tapeset(1, 256, table=tid),
                                            [0, 1], tabs, lookup_cases.key_soa(keys, 1), native)
        tab, els, _ = tabs[tid]
        assert got[0] == [fake_tables.lookup_ref(tab, els, k) for k in keys]
        assert got[1] == [fake_tables.lookup_ref(tab, els, k, hit=True) for k in keys]


def test_cpp_step_library(gpu_ctx):
    """The MH_ASM_CORE=0 library runs D_LOOKUP through the same step() (one child process with
    MYTHRIL_HIP_LIB naming it: tests/noasm_lookup_check.py)."""
    lib = os.path.join(ROOT, "mythril_amd", "libmythril_hip_noasm.so")
    assert os.path.exists(lib), "build it first: make -C mythril_amd/csrc noasm (build() does)"
    r = subprocess.run([sys.executable, "-u", "-m", "tests.noasm_lookup_check"], cwd=ROOT,
                       env=dict(os.environ, MYTHRIL_HIP_LIB=lib), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "noasm lookup ok" in r.stdout


def test_other_entry_points_refuse_table_tapes(gpu_ctx):
    ts = lookup_cases.lookup_tapeset(1, 256)
    ct = gpu_ctx.compile(ts)
    a = gpu_ctx.assignments(ts.n_vars, 64)
    a.upload(lookup_cases.key_soa(list(range(64)), 1))
    try:
        before = native.eval_launches(gpu_ctx)
        for call in (lambda: native.run(gpu_ctx, ct, a),
                     lambda: native.run_rows(gpu_ctx, ct, a, 1),
                     lambda: native.eval_values_many(gpu_ctx, ct, [0], a, 0),
                     lambda: native.eval_values(gpu_ctx, ct, 0, a),
                     lambda: ct.jit()):
            with pytest.raises(native.Unsupported) as e:
                call()
            assert e.value.code == native.MH_E_UNSUPPORTED and "lookup" in str(e.value)
        assert native.eval_launches(gpu_ctx) == before  # nothing was launched
        # a table set without the table the tape names, and one with another key width
        for tabs in ([], [({}, 0, 512)]):
            tb = native.tables_create(gpu_ctx, tabs)
            try:
                with pytest.raises(native.SieveError) as e:
                    native.eval_values_tables(gpu_ctx, ct, tb, [0], a, 0, 64)
                assert e.value.code == native.MH_E_INVALID
            finally:
                tb.close()
        assert native.eval_launches(gpu_ctx) == before
    finally:
        a.close()
        ct.close()


def test_tables_create_refuses_unsorted_keys(gpu_ctx):
    import ctypes as C

    raw = list(native.pack_tables([({3: 1, 5: 2}, 0, 256)]))

    def create():  # mh_tables_create on the arrays as they stand
        counts, nws, koffs, keys, voffs, vals, elses, n_keys, n_vals = raw
        h = C.c_void_p()
        p = native._ptr
        r = gpu_ctx.lib.mh_tables_create(gpu_ctx.h, 1, p(counts), p(nws), p(koffs, C.c_uint64),
                                         p(keys), n_keys, p(voffs, C.c_uint64), p(vals), n_vals,
                                         p(elses), C.byref(h))
        if r == native.MH_OK:
            gpu_ctx.lib.mh_tables_destroy(h)
        return r, gpu_ctx.lib.mh_last_error().decode()

    assert create()[0] == native.MH_OK
    keys = raw[3].copy()
    keys[0], keys[8] = 5, 3  # descending
    raw[3] = keys
    r, msg = create()
    assert r == native.MH_E_INVALID and "ascending" in msg
    keys[0] = 3  # repeated
    assert create()[0] == native.MH_E_INVALID
    keys[0], keys[8] = 3, 5
    assert create()[0] == native.MH_OK
    raw[1] = np.array([4], dtype=np.uint32)  # four key words
    r, msg = create()
    assert r == native.MH_E_INVALID and "1..3" in msg
