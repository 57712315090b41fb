"""Inline division paths of the tape JIT (jit.cpp op_div, MH_JIT_DIV) on the host wave emulator.

Every tape of tests/div_cases.py gives the C oracle's value on every row at every MH_JIT_DIV
level, and the emulator's count of executed division calls tells which side of each site ran:
none in the waves built for a hot path, one per wave built to fall back, one per wave and site
with MH_JIT_DIV=0."""
import ctypes as C

import pytest

from mythril_amd import synth
from oracle import ctape, smt_eval
from tests import div_cases as dc
from tests.emu import jit_eval
from tests.test_jit import soa_of

LEVELS = ("0", "1", "2", "3", None)


@pytest.fixture(scope="module")
def cases():
    return dc.build()


def set_level(monkeypatch, level):
    monkeypatch.delenv("MH_JIT_STAGE", raising=False)
    if level is None:
        monkeypatch.delenv("MH_JIT_DIV", raising=False)
    else:
        monkeypatch.setenv("MH_JIT_DIV", level)


def calls(emu, reset=True):
    """Division calls the emulator has executed since the last reset (emu_jit_div_hist)."""
    f = emu.lib.emu_jit_div_hist
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    h = (C.c_uint64 * 32)()
    f(h, int(reset))
    return sum(h)


def run(emu, ts, tape, soa, want):
    calls(emu)
    res = jit_eval(emu, ts, tape, soa)
    assert res.ok, res.why
    bad = [r for r in range(len(want)) if res.values[r] != want[r]]
    assert not bad, (tape, bad[:4], hex(res.values[bad[0]]), hex(want[bad[0]]))
    return calls(emu)


def oracle(ts, tape, rows):
    return [ctape.evaluate(ts, tape, r) for r in rows]


def inline_level(path):
    """The lowest MH_JIT_DIV level at which a site of this path is inline (99: never)."""
    return {1: 1, "fold": 1, 3: 3}.get(path, 99)


def check_waves(emu, monkeypatch, ts, name, entry, waves, path):
    """Tape `name` over the waves of inline path `path`: values at every level, and the calls the
    waves' kinds predict -- a site is called in every wave unless it is inline at that level,
    and an inline site of `path` is called in the cold waves (for a values tape, which has no
    guard, also in the waves whose undecided lane the guard would kill)."""
    tape, paths = entry
    rows, kinds = dc.flatten(waves)
    soa = soa_of(rows, ts.n_vars)
    want = oracle(ts, tape, rows)
    fall = sum(1 for k in kinds if k == dc.COLD or (k == dc.DEAD and name.endswith("_v")))
    for level in LEVELS:
        set_level(monkeypatch, level)
        lv = 3 if level is None else int(level)
        expect = 0
        for p in paths:
            if inline_level(p) > lv:
                expect += len(kinds)
            elif p == path:
                expect += fall
        got = run(emu, ts, tape, soa, want)
        assert got == expect, (name, level, got, expect)


@pytest.mark.parametrize("op", ["udiv", "urem", "sdiv", "srem", "smod"])
@pytest.mark.parametrize("shape", ["c32_var", "x160_var"])
def test_short_dividend(emu, monkeypatch, cases, shape, op):
    ts, idx = cases
    waves = dc.path1_waves(21, op[0] == "s")
    for suffix in ("_v", "_b"):
        name = "%s_%s%s" % (shape, op, suffix)
        check_waves(emu, monkeypatch, ts, name, idx[name], waves, 1)


@pytest.mark.parametrize("op", ["udiv", "urem", "sdiv", "srem", "smod"])
def test_small_quotient(emu, monkeypatch, cases, op):
    ts, idx = cases
    waves = dc.path3_waves(22, op[0] == "s")
    for suffix in ("_v", "_b"):
        name = "var_var_%s%s" % (op, suffix)
        check_waves(emu, monkeypatch, ts, name, idx[name], waves, 3)


@pytest.mark.parametrize("name", ["two_p1_call_v", "two_p3_call_v", "two_call_p3_v",
                                  "two_p1_p3_b", "lowlimb_udiv_v", "lowlimb_sdiv_v"])
def test_two_sites_and_partial_demand(emu, monkeypatch, cases, name):
    """Hot waves of the small-quotient path (their divisors' top limbs are nonzero, so a
    short-dividend site is hot on them too): only the called site calls."""
    ts, idx = cases
    signed = "sdiv" in name or name == "two_call_p3_v"
    waves = [w for w in dc.path3_waves(23, signed) if w[0] == dc.HOT]
    tape, paths = idx[name]
    rows, kinds = dc.flatten(waves)
    soa = soa_of(rows, ts.n_vars)
    want = oracle(ts, tape, rows)
    for level in LEVELS:
        set_level(monkeypatch, level)
        lv = 3 if level is None else int(level)
        expect = sum(len(kinds) for p in paths if inline_level(p) > lv)
        assert run(emu, ts, tape, soa, want) == expect, (name, level)
    # and with the cold waves: values only
    rows, _ = dc.flatten(dc.path3_waves(23, signed))
    want = oracle(ts, tape, rows)
    for level in ("0", None):
        set_level(monkeypatch, level)
        run(emu, ts, tape, soa_of(rows, ts.n_vars), want)


def test_every_tape_on_general_rows(emu, monkeypatch, cases):
    """Every shape -- the called ones, the compile-time fold, x / x -- on rows with each digit on
    an integer boundary, zero and all-ones operands and the signed corners, at every level; the
    plain build calls at every site of every live wave, the fold never."""
    ts, idx = cases
    rows = dc.general_rows(24)
    soa = soa_of(rows, ts.n_vars)
    n_waves = (len(rows) + 63) // 64
    for name, (tape, paths) in idx.items():
        want = oracle(ts, tape, rows)
        got = {}
        for level in LEVELS:
            set_level(monkeypatch, level)
            got[level] = run(emu, ts, tape, soa, want)
        assert got["0"] == n_waves * len(paths), (name, got)
        if paths == ["fold"]:
            assert got["1"] == got[None] == 0, (name, got)
        if all(p == 0 for p in paths):
            assert got[None] == got["0"], (name, got)


def test_stage_switch_turns_it_off(emu, monkeypatch, cases):
    """MH_JIT_STAGE=0 asks for the plain code: the inline paths go with it."""
    ts, idx = cases
    tape, _ = idx["c32_var_udiv_v"]
    rows, kinds = dc.flatten(dc.path1_waves(21, False)[:1])
    want = oracle(ts, tape, rows)
    monkeypatch.delenv("MH_JIT_DIV", raising=False)
    monkeypatch.setenv("MH_JIT_STAGE", "0")
    assert run(emu, ts, tape, soa_of(rows, ts.n_vars), want) == len(kinds)


def test_config5_levels_agree(emu, monkeypatch):
    """Config-5 tapes 0-299 x 128 generated rows: identical values at levels 0 and 3, and the
    default level runs fewer division calls."""
    ts = synth.generate(300)
    seed = synth.load_spec()["assignment_seed"]
    soa = soa_of([smt_eval.gen_assignment(seed, ts.n_vars, r) for r in range(128)], ts.n_vars)
    vals, n_calls = {}, {}
    for level in ("0", "3"):
        set_level(monkeypatch, level)
        calls(emu)
        vals[level] = [jit_eval(emu, ts, i, soa).values for i in range(len(ts.tapes))]
        n_calls[level] = calls(emu)
    assert vals["0"] == vals["3"]
    assert sum(v is not None for v in vals["3"]) >= 290
    print("division calls", n_calls)
    assert n_calls["3"] < 0.75 * n_calls["0"], n_calls
