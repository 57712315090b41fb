"""The repair step's device kernels (csrc/repair.hip behind mh_repair_score / _select / _mutate)
against their CPU restatement (tests/repair_ref.py), bit for bit, at the shapes where they can go
wrong; and Sieve's repair policy on the device against the same policy on the CPU stand-in."""
import random

import numpy as np
import pytest

from mythril_amd import native
from mythril_amd.sieve import Sieve
from mythril_amd.tape import Op, TapeSet
from oracle import smt_eval as E
from tests import repair_ref
from tests.fuzz import TapeFuzzer, assignment_soa, soa_row, tree_tape
from tests.repair_cases import chain_query
from tests.test_gpu_frontend import _random_guide
from tests.test_reference_fixtures import holds_original

pytestmark = pytest.mark.gpu

N_TAPES, N_ROWS = 133, 4200


@pytest.fixture(scope="module")
def scoring(gpu_ctx):
    """133 Bool tapes over 3 columns -- fuzzed at depths 1..4 with the EVM helpers and overflow
    predicates (complex-op kernel variants) between plain comparisons (the asm-only variant) and
    wide expression trees (the 9- and 15-register classes) -- compiled once, rows of edge-biased
    values uploaded once, and a memo of the reference's (tape, row) values shared by the cases."""
    rng = random.Random(0x5C0)
    ts = TapeSet()
    fz = TapeFuzzer(rng, ts, n_vars=3, allow_keccak=False, max_depth=4)
    b = fz.b
    for i in range(N_TAPES):
        if i % 16 == 5:    # 8 registers: the middle class
            tree_tape(ts, b, 5, i)
        elif i % 32 == 9:  # 10 registers: the largest class
            tree_tape(ts, b, 7, i)
        elif i % 3 == 0:  # short tapes: few registers, no complex op
            v = b.var("v%d" % (i % 3), 256)
            ts.add(b.finish(b.op(Op.BVULT, v, b.const(1 << (8 * (i % 31) + 3), 256))))
        else:
            fz.max_depth = 1 + i % 4
            fz.tape(root_bool=True)
    ct = gpu_ctx.compile(ts)
    info = ct.info()
    classes = {native_nr_class(x["n_regs"]) for x in info}
    assert len(classes) >= 2, "the tapes must launch at least two register classes"
    # keccak / EVM helpers / other C++ ops (dev_isa.h F_*): a complex-op variant, and a plain one
    assert any(x["features"] & 14 for x in info) and any(not x["features"] & 14 for x in info)
    soa = assignment_soa(rng, 3, N_ROWS)
    a = gpu_ctx.assignments(3, N_ROWS)
    a.upload(soa)
    rows = [soa_row(soa, r) for r in range(N_ROWS)]
    memo = {}

    def fails(tape_first, tape_count, row_first, row_count):
        out = []
        for r in range(row_first, row_first + row_count):
            line = []
            for t in range(tape_first, tape_first + tape_count):
                if (t, r) not in memo:
                    memo[t, r] = not bool(E.evaluate(ts.tapes[t].nodes, ts.pool.values, rows[r]))
                line.append(memo[t, r])
            out.append(line)
        return out

    rep = native.repair_open(gpu_ctx, 160, 1 << 16, 256)
    yield ct, a, fails, rep
    rep.close()
    a.close()
    ct.close()


def native_nr_class(n_regs):  # csrc/kernels.h nr_class
    return 0 if n_regs <= 7 else 1 if n_regs <= 9 else 2


# conjunct counts across the interpreter's 64-tape LDS chunk, rows across the one-wave (<= 4096
# rows) and 256-thread workgroup forms and their partial last waves, row_first != 0
SCORE_CASES = [(0, 2, 0, 1), (1, 64, 1, 63), (0, 64, 3, 64), (3, 65, 0, 65), (0, 130, 5, 257),
               (2, 130, 9, 65), (130, 2, 7, 4097), (66, 3, 100, 4100)]


@pytest.mark.parametrize("tape_first,tape_count,row_first,row_count", SCORE_CASES)
def test_score_matches_reference(scoring, tape_first, tape_count, row_first, row_count):
    ct, a, fails, rep = scoring
    got = native.repair_score(rep, ct, a, tape_first=tape_first, tape_count=tape_count,
                              row_first=row_first, row_count=row_count, counts=True)
    want = [sum(f) for f in fails(tape_first, tape_count, row_first, row_count)]
    assert got.tolist() == want
    if row_count >= 63:
        assert 0 < sum(want) < tape_count * row_count  # neither all true nor all false


def check_select(rep, fails, row_first, k, seed):
    got = native.repair_select(rep, k, seed)
    want = repair_ref.select(fails, row_first, k, seed)
    assert [tuple(int(x) for x in e) for e in got.tolist()] == want
    return want


def test_select_after_a_wide_score(scoring):
    """130 conjuncts: many distinct counts below the threshold, placed by (count, row)."""
    ct, a, fails, rep = scoring
    native.repair_score(rep, ct, a, tape_first=0, tape_count=130, row_first=5, row_count=257)
    f = fails(0, 130, 5, 257)
    for k, seed in ((1, 1), (64, 2), (256, 3)):
        check_select(rep, f, 5, k, seed)


@pytest.fixture(scope="module")
def bits(gpu_ctx):
    """Five conjuncts v_i == 1 over 2^16 rows of 0 / 1 columns: the fail counts are the rows'
    zero columns, so the reference is a table look-up."""
    ts = TapeSet()
    b = ts.builder()
    for i in range(5):
        ts.add(b.finish(b.op(Op.EQ, b.var("v%d" % i, 256), b.const(1, 256))))
    ct = gpu_ctx.compile(ts)
    rng = np.random.default_rng(77)
    n = 1 << 16
    soa = np.zeros((12, 8, n), dtype=np.uint32)  # columns 5.. are beyond the tapes' (and a guide's)
    soa[:5, 0, :] = rng.random((5, n)) < 0.3
    soa[5:, :, :] = rng.integers(0, 1 << 32, size=(7, 8, n), dtype=np.uint64).astype(np.uint32)
    soa[:5, 0, 300:600] = 0          # a run of all-equal scores (every conjunct fails)
    soa[:5, 0, 40000] = 1            # rows that fail nothing
    soa[:5, 0, 7] = 1
    a = gpu_ctx.assignments(12, n)
    a.upload(soa)
    rep = native.repair_open(gpu_ctx, 8, n, 256)
    yield ct, a, soa, rep
    rep.close()
    a.close()
    ct.close()


def bit_fails(soa, row_first, row_count):
    return [[int(soa[c, 0, r]) != 1 for c in range(5)]
            for r in range(row_first, row_first + row_count)]


@pytest.mark.parametrize("row_first,row_count,k", [
    (0, 1 << 16, 1), (0, 1 << 16, 256),   # the extremes over the largest run
    (11, 100, 256),                       # k > rows: every row, ordered
    (300, 300, 64),                       # all-equal scores: the lowest rows
    (1, 4097, 200), (0, 64, 64)])
def test_select_matches_reference(bits, row_first, row_count, k):
    ct, a, soa, rep = bits
    got = native.repair_score(rep, ct, a, row_first=row_first, row_count=row_count, counts=True)
    f = bit_fails(soa, row_first, row_count)
    assert got.tolist() == [sum(x) for x in f]
    want = check_select(rep, f, row_first, k, 0xABC + k)
    assert len(want) == min(k, row_count)
    if (row_first, row_count) == (300, 300):
        assert [e[0] for e in want] == list(range(300, 300 + k))
    if row_count == 1 << 16:  # a row that fails nothing comes first, with no pick
        assert want[0][1:] == (0, native.NO_CONJUNCT) and want[0][0] <= 7


def mutate_case(bits, gpu_ctx, flags, seed):
    """Elites of rows [0, 4096) (one fails nothing: all copies), children in a second buffer."""
    ct, a, soa, rep = bits
    rng = np.random.default_rng(1000 + seed)
    arrays = _random_guide(rng, 9, 40)        # 9 of the buffer's 12 columns; widths 1..256
    arrays["width"][:4] = [8, 160, 256, 1]
    n_sets = len(arrays["set_off"]) - 1
    # conjunct 3 has no set (the redraw path); some sets belong to no conjunct
    tags = rng.choice([0, 1, 2, 4, native.NO_CONJUNCT], size=n_sets).astype(np.uint32)
    conj_cols = [sorted(rng.choice(9, size=int(rng.integers(1, 4)), replace=False).tolist())
                 for _ in range(5)]
    col_off = np.concatenate([[0], np.cumsum([len(c) for c in conj_cols])]).astype(np.uint32)
    cols = np.array([c for cc in conj_cols for c in cc], dtype=np.uint32)
    native.repair_score(rep, ct, a, row_first=0, row_count=4096)
    el = native.repair_select(rep, 48, seed)
    elites = [tuple(int(x) for x in e) for e in el.tolist()]
    assert elites[0][2] == native.NO_CONJUNCT and {e[2] for e in elites} >= {0, 1, 2, 3, 4}
    per, base = 5, (1 << 33) + 17
    dst = gpu_ctx.assignments(12, len(elites) * per + 3)
    try:
        native.repair_mutate(rep, a, dst, arrays, tags, col_off, cols, per, flags=flags,
                             seed=seed, global_base=base)
        got = dst.download(0, len(elites) * per)
    finally:
        dst.close()
    want = repair_ref.mutate(lambda r: soa_row(soa, r), elites, arrays, tags, conj_cols, per,
                             flags, seed, base)
    for i, row in enumerate(want):
        assert soa_row(got, i) == row, (i, elites[i // per])
    return elites, want


def test_mutate_matches_reference(bits, gpu_ctx):
    elites, want = mutate_case(bits, gpu_ctx, 0, 5)
    src_rows = {e[0] for e in elites}
    assert len(src_rows) == len(elites)
    changed = sum(want[s * 5 + c] != want[s * 5] for s in range(len(elites)) for c in range(1, 5))
    assert changed > len(elites)  # the children differ from their elites


def test_mutate_redraw_matches_reference(bits, gpu_ctx):
    mutate_case(bits, gpu_ctx, native.MUTATE_REDRAW, 6)


def test_refusals_before_any_launch(bits, gpu_ctx):
    ct, a, soa, rep = bits
    arrays = _random_guide(np.random.default_rng(3), 9, 4)
    tags = np.zeros(4, dtype=np.uint32)
    col_off = np.array([0, 1, 2, 3, 4, 5], dtype=np.uint32)
    cols = np.arange(5, dtype=np.uint32)
    native.repair_score(rep, ct, a, row_first=0, row_count=64)
    native.repair_select(rep, 8, 1)
    small = gpu_ctx.assignments(12, 16)
    narrow = gpu_ctx.assignments(9, 64)
    try:
        def refused(fn):
            with pytest.raises(native.SieveError) as e:
                fn()
            assert e.value.code == native.MH_E_INVALID

        refused(lambda: native.repair_mutate(rep, a, a, arrays, tags, col_off, cols, 2))
        refused(lambda: native.repair_mutate(rep, a, small, arrays, tags, col_off, cols, 3))
        refused(lambda: native.repair_mutate(rep, a, narrow, arrays, tags, col_off, cols, 2))
        refused(lambda: native.repair_mutate(rep, a, small, arrays, tags, col_off,
                                             cols + 9, 2))           # a column outside the guide
        refused(lambda: native.repair_mutate(rep, a, small, arrays, tags + 5, col_off, cols, 2))
        refused(lambda: native.repair_select(rep, 257, 1))
        refused(lambda: native.repair_score(rep, ct, a, row_first=0, row_count=(1 << 16) + 1))
        refused(lambda: native.repair_score(rep, ct, a, tape_first=0, tape_count=9))
        refused(lambda: native.repair_open(gpu_ctx, 4097, 64, 8))
        refused(lambda: native.repair_open(gpu_ctx, 8, (1 << 16) + 1, 8))
        refused(lambda: native.repair_open(gpu_ctx, 8, 64, 257))
        native.repair_mutate(rep, a, small, arrays, tags, col_off, cols, 2)  # 8 x 2 rows fit
    finally:
        small.close()
        narrow.close()


def test_chain_query_as_on_the_stand_in(gpu_ctx):
    """The M = 6 chain through Sieve on the device: a miss without repair, and with repair the
    stand-in's witness after the stand-in's number of iterations."""
    kw = dict(rows=256, first_rows=256, max_rounds=1, keccak_second_chance=False, budget_s=600.0)
    rk = dict(repair_rounds=8, repair_elites=8, repair_children=8)

    def run(**more):
        ctx, cs = chain_query(6)
        s = Sieve(**dict(kw, **more))
        try:
            w = s.solve(ctx.b, [c.node for c in cs])
            return ctx, cs, w, dict(s.stats.extra)
        finally:
            s.close()

    mp = pytest.MonkeyPatch()
    try:
        repair_ref.install(mp)
        _, _, fw0, _ = run()
        _, _, fw, fextra = run(**rk)
    finally:
        mp.undo()
    assert fw0 is None and fw is not None
    _, _, w0, extra0 = run()
    assert w0 is None and not [k for k in extra0 if k.startswith("repair")]
    ctx, cs, w, extra = run(**rk)
    assert w is not None and w.repaired
    assert w.values == fw.values and w.index == fw.index
    assert extra["repair_iters"] == fextra["repair_iters"]
    assert holds_original(ctx, cs, w.schema, w.values)
