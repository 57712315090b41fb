"""Jobs for the mh_eval_values_jobs tests (test helper): shared by tests/test_gpu_values_jobs.py
and tests/noasm_values_jobs_check.py (the C++ step() library).  Every job is checked against the
single call it stands for: native.eval_values_tables at one row, or native.eval_values_many when
it has no tables.  The tapes are those of tests/lookup_cases.py plus table-free ones."""
import numpy as np

from mythril_amd.tape import Op, TapeSet
from tests import lookup_cases

LIVES = (0, 6, 10)  # lookup_cases.lookup_tapeset's `live` for the NR 7 / 9 / 15 kernels


def plain_tapeset(n_simple=3):
    """Table-free tapes over column k0: `n_simple` sums k0 + i, then per register class a mix of
    products that stay live (asm-only variants), then a keccak tape and a division tape."""
    ts = TapeSet()
    b = ts.builder()
    x = b.var("k0", 256)
    for i in range(n_simple):
        ts.add(b.finish(b.op(Op.BVADD, x, b.const(i + 1, 256))))
    for live in LIVES[1:]:
        vs = [b.op(Op.BVMUL, x, b.const(0x9E3779B97F4A7C15 + 2 * i, 256)) for i in range(live)]
        s1, s2 = vs[0], x
        for v in vs[1:]:
            s1 = b.op(Op.BVADD, s1, v)
        for v in vs:
            s2 = b.op(Op.BVXOR, b.op(Op.BVMUL, s2, v), v)
        ts.add(b.finish(b.op(Op.BVXOR, s1, s2)))
    ts.add(b.finish(b.op(Op.BVLSHR, b.op(Op.KECCAK, x), b.const(139, 256))))
    ts.add(b.finish(b.op(Op.BVUDIV, x, b.op(Op.BVOR, b.op(Op.BVLSHR, x, b.const(200, 256)),
                                             b.const(1, 256)))))
    return ts


class Handles:
    """Compiled tape sets, buffers and table sets of a test, closed together."""

    def __init__(self, ctx, native):
        self.ctx, self.native, self.open = ctx, native, []

    def compile(self, ts):
        ct = self.ctx.compile(ts)
        self.open.append(ct)
        return ct

    def assign(self, n_vars, keys_per_row, nw_per_row=None, capacity=None):
        """A buffer of `n_vars` columns whose row r holds key keys_per_row[r] in its first
        columns (nw_per_row[r] of them, default n_vars)."""
        rows = len(keys_per_row)
        soa = np.zeros((n_vars, 8, rows), dtype=np.uint32)
        for r, k in enumerate(keys_per_row):
            nw = n_vars if nw_per_row is None else nw_per_row[r]
            soa[:nw, :, r] = lookup_cases.key_soa([k], nw)[:, :, 0]
        a = self.ctx.assignments(n_vars, capacity or rows)
        self.open.append(a)
        a.upload(soa)
        return a

    def tables(self, tabs):
        tb = self.native.tables_create(self.ctx, tabs)
        self.open.append(tb)
        return tb

    def close(self):
        for h in reversed(self.open):
            h.close()
        self.open = []


def single(ctx, native, job):
    """What the job's single call gives: u32 [len(ids), 8]."""
    ct, tb, ids, a, row = job
    if tb is None:
        return native.eval_values_many(ctx, ct, ids, a, row)
    return native.eval_values_tables(ctx, ct, tb, ids, a, row, 1)[:, :, 0]


def check_jobs(ctx, native, jobs):
    """One eval_values_jobs over `jobs` against every job's single call, bit for bit."""
    got = native.eval_values_jobs(ctx, jobs)
    assert len(got) == len(jobs)
    for i, job in enumerate(jobs):
        want = single(ctx, native, job)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), i
    return got


def mixed_jobs(h):
    """One list mixing all three register classes, table and table-free variants, a keccak tape
    and a complex-op tape, keys of 1, 2 and 3 words, an empty table, repeated and descending ids,
    a job of one tape; returns (jobs, the variants' (n_regs class, has table) seen)."""
    jobs, seen = [], set()

    def note(ct, ids):
        info = ct.info()
        for t in ids:
            nr = int(info[t]["n_regs"])
            seen.add((0 if nr <= 7 else 1 if nr <= 9 else 2, bool(int(info[t]["features"]) & 16)))

    for nw in (1, 2, 3):
        rng = lookup_cases.case_rng(9000, nw)
        table, els = lookup_cases.make_table(rng, 65, nw, 160)
        keys = lookup_cases.probes(rng, table, nw, 4)
        ct = h.compile(lookup_cases.lookup_tapeset(nw, 160))
        a = h.assign(nw, keys)
        tb = h.tables([(table, els, 256 * nw)])
        empty = h.tables([({}, 0x55 + nw, 256 * nw)])
        jobs += [(ct, tb, [2, 1, 0, 2], a, 1), (ct, empty, [0, 1], a, 3), (ct, tb, [1], a, 0)]
        note(ct, [0, 1, 2])
        if nw == 2:  # the lookup among live registers: the NR 9 and NR 15 table kernels
            for live in LIVES[1:]:
                ct = h.compile(lookup_cases.lookup_tapeset(nw, 160, live=live))
                jobs.append((ct, tb, [2, 0], a, 2))
                note(ct, [2])
    rng = lookup_cases.case_rng(9001)
    table, els = lookup_cases.make_table(rng, 64, 1, 256)
    keys = sorted(table)[:2] + [7]
    ct = h.compile(lookup_cases.mixed_tapeset())
    tb, a = h.tables([(table, els, 256)]), h.assign(1, keys)
    jobs += [(ct, tb, [1, 0, 1, 1, 0], a, r) for r in range(3)]
    pts = plain_tapeset()
    ct = h.compile(pts)
    note(ct, range(len(pts.tapes)))
    a = h.assign(1, [rng.getrandbits(256) for _ in range(3)])
    n = len(pts.tapes)
    jobs += [(ct, None, list(range(n - 1, -1, -1)) + [0, n - 1, 0], a, 2), (ct, None, [n - 2], a, 0),
             (ct, None, [], a, 1)]
    return jobs, seen
