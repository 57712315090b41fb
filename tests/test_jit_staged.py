"""Staged conjuncts of the tape JIT (jit.cpp emit_staged) on the host wave emulator: a conjunct
that is a 256-bit compare is decided from one limb of each operand where it can be, and falls
back to the full cone where a live lane is undecided.  Every tape runs with MH_JIT_STAGE=0 (the
plain code) and at the default level; both must give the oracle's root on every row, and the
emulator's executed-VALU count tells which path ran."""
import pytest

from mythril_amd import native, synth
from oracle import smt_eval
from tests import staged_cases as sc
from tests.emu import jit_eval
from tests.fuzz import soa_row
from tests.test_jit import soa_of

LEVEL0_BUILD = "bfac4c49aa97d03b"  # config-5 code id of the plain short-circuit build


@pytest.fixture(scope="module")
def cases():
    return sc.build()


def oracle(ts, tape, rows):
    soa = soa_of(rows, ts.n_vars)
    return [int(smt_eval.evaluate(ts.tapes[tape].nodes, ts.pool.values, soa_row(soa, r)))
            for r in range(len(rows))]


def run_levels(emu, monkeypatch, ts, tape, rows, want=None):
    """Executed VALU per wave at (level 0, default level); roots checked against the oracle."""
    soa = soa_of(rows, ts.n_vars)
    want = want or oracle(ts, tape, rows)
    valu = []
    for level in ("0", None):
        if level is None:
            monkeypatch.delenv("MH_JIT_STAGE", raising=False)
        else:
            monkeypatch.setenv("MH_JIT_STAGE", level)
        res = jit_eval(emu, ts, tape, soa)
        assert res.ok, res.why
        bad = [r for r in range(len(rows)) if res.values[r] != want[r]]
        assert not bad, (level, tape, bad[:4], [hex(v) for v in rows[bad[0]]])
        valu.append(res.dyn["valu"])
    return valu[0], valu[1], want


def test_eq_over_multiplication(emu, monkeypatch, cases):
    ts, idx = cases
    t = idx["eq_mul"]
    rows = sc.rows_eq_mul()
    # (a) no equal low limbs: the slice decides, the product's other limbs are never computed
    v0, v1, want = run_levels(emu, monkeypatch, ts, t, rows["a"])
    assert not any(want) and v1 < v0 - 30, (v0, v1)
    hot = v1
    # (b) equal low limbs, unequal high limbs: the fallback runs, the row is false
    v0, v1, want = run_levels(emu, monkeypatch, ts, t, rows["b"])
    assert not any(want) and v1 > hot + 30, (v0, v1, hot)
    # (c) equal in every limb: the fallback runs, the row is true
    v0, v1, want = run_levels(emu, monkeypatch, ts, t, rows["c"])
    assert want[17] == 1 and sum(want) == 1 and v1 > hot + 30, (v0, v1, hot)
    # (d) equal low limbs in a row an earlier conjunct killed: no fallback
    v0, v1, want = run_levels(emu, monkeypatch, ts, t, rows["d"])
    assert not any(want) and v1 == hot, (v0, v1, hot)


@pytest.mark.parametrize("name", ["ult", "ule", "ugt", "uge", "slt", "sle", "sgt", "sge"])
def test_ordered_over_logic_cone(emu, monkeypatch, cases, name):
    ts, idx = cases
    t = idx["logic_" + name]
    # top limbs differ in every live lane: decided from the top-limb slice of the cone
    v0, hot, want = run_levels(emu, monkeypatch, ts, t, sc.rows_decided())
    assert 0 < sum(want) < 64 and hot < v0 - 8, (v0, hot)
    # equal top limbs, equal operands, the signed boundary: the fallback decides
    v0, v1, want = run_levels(emu, monkeypatch, ts, t, sc.rows_ordered())
    assert 0 < sum(want) < 64 and v1 > hot, (v0, v1, hot)


@pytest.mark.parametrize("name", ["add_ult", "sub_uge", "add_slt", "chain3_ult", "chain3_sge",
                                  "both_sides", "ite_sums", "sum_and"])
def test_carry_slack(emu, monkeypatch, cases, name):
    """Top limbs computed with the carry-in left open: rows on, next to and far from the compared
    top limb, and on the wrap of the top limb, with and without a carry out of limb 6."""
    ts, idx = cases
    t = idx[name]
    for rows in (sc.rows_carry(False), sc.rows_carry(True)):
        run_levels(emu, monkeypatch, ts, t, rows)
    # each crafted row alone in a wave of far-apart rows: a lane wrongly taken as decided is not
    # rescued by another lane's fallback
    base = sc.rows_far()
    v0, hot, want_base = run_levels(emu, monkeypatch, ts, t, base)
    if name == "chain3_ult":  # far apart: no fallback, the carry chains are never run
        assert hot < v0 - 8, (v0, hot)
    for h in sc.hazard_rows():
        rows = [h] + base[1:]
        run_levels(emu, monkeypatch, ts, t, rows, oracle(ts, t, [h]) + want_base[1:])


@pytest.mark.parametrize("name", ["shared", "shared_ord"])
def test_shared_cone(emu, monkeypatch, cases, name):
    """A node used by the staged conjunct and by a later one is computed in full before the
    slice: the later conjunct reads it on rows where the slice decided."""
    ts, idx = cases
    t = idx[name]
    rng_rows = sc.rows_decided() if name == "shared_ord" else sc.rows_eq_mul()["a"]
    rows = [list(r) for r in rng_rows]
    if name == "shared":  # some rows pass the staged == so that the later conjunct decides
        for r in range(0, 64, 3):
            xv, yv, zv = rows[r][:3]
            # shared = ((p + z) ^ (z << 40)) + x == z  <=>  p = ((z - x) ^ (z << 40)) - z
            p = ((((zv - xv) & sc.M) ^ ((zv << 40) & sc.M)) - zv) & sc.M
            if xv % 2 == 0:
                xv |= 1
                p = ((((zv - xv) & sc.M) ^ ((zv << 40) & sc.M)) - zv) & sc.M
            rows[r][0], rows[r][1] = xv, (p * pow(xv, -1, 1 << 256)) & sc.M
    v0, v1, want = run_levels(emu, monkeypatch, ts, t, rows)
    if name == "shared":
        assert any((((r[0] * r[1] + r[2]) ^ (r[2] << 40)) + r[0]) & sc.M == r[2] for r in rows)
    else:
        assert 0 < sum(want) < 64


def test_every_case_on_every_row_set(emu, monkeypatch, cases):
    ts, idx = cases
    for rows in (sc.rows_ordered(), sc.rows_decided(), sc.rows_wrap(False), sc.rows_wrap(True)):
        for t in range(len(ts.tapes)):
            run_levels(emu, monkeypatch, ts, t, rows)


def test_config5_slice(emu, monkeypatch):
    """Config-5 tapes 0-199 x 256 generated rows at the default level, against the oracle."""
    monkeypatch.delenv("MH_JIT_STAGE", raising=False)
    ts = synth.generate(200)
    seed = synth.load_spec()["assignment_seed"]
    soa = soa_of([smt_eval.gen_assignment(seed, ts.n_vars, r) for r in range(256)], ts.n_vars)
    assigns = [soa_row(soa, r) for r in range(256)]
    n = 0
    for i, t in enumerate(ts.tapes):
        res = jit_eval(emu, ts, i, soa)
        if not res.ok:
            continue
        n += 1
        for r in range(256):
            want = int(smt_eval.evaluate(t.nodes, ts.pool.values, assigns[r]))
            assert res.values[r] == want, (i, r)
    assert n >= 190


def test_level0_is_the_plain_build(monkeypatch):
    """MH_JIT_STAGE=0 emits the code of the build before staging, module text for module text."""
    monkeypatch.setenv("MH_JIT_STAGE", "0")
    assert native.jit_code_id(synth.generate()) == LEVEL0_BUILD
