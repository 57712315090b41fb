"""Width-specialised variants of the division subroutine (jit.cpp op_div / div_routine,
MH_JIT_STAGE=5) on the host wave emulator.

Every tape of tests/div_width_cases.py gives the C oracle's value on every row at MH_JIT_STAGE 4,
5 and unset and with MH_JIT_DIV=0 (the emulator's v_rcp_f64 is the approximate one, 22 mantissa
bits, in every run: the Newton steps and the host-rounded reciprocals are what is under test).
The emulator's label counts say which code ran -- a hot wave enters no legacy L_UNS, a wave with
one short-divisor lane exactly one -- and its op statistics that the hot waves execute fewer f64
ops than at level 4.  The old level keeps its build id, and a module without a variant site its
text."""
import ctypes as C

import pytest

from mythril_amd import native, synth
from mythril_amd.tape import Op, TapeSet
from oracle import ctape, smt_eval
from tests import div_width_cases as wc
from tests.emu import jit_eval, jit_module
from tests.test_jit import soa_of

L_UNS = 1
# (MH_JIT_STAGE, MH_JIT_DIV)
CONFIGS = (("4", None), ("5", None), (None, None), (None, "0"))


@pytest.fixture(scope="module")
def cases():
    return wc.build()


def configure(monkeypatch, stage, div):
    for name, v in (("MH_JIT_STAGE", stage), ("MH_JIT_DIV", div)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def legacy_entries(emu):
    """Entries of the legacy code (label L_UNS) since the last call (emu_jit_div_labels)."""
    f = emu.lib.emu_jit_div_labels
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    h = (C.c_uint64 * 128)()
    f(h, 1)
    return int(h[L_UNS])


def run(emu, ts, tape, soa, want, tag):
    legacy_entries(emu)
    res = jit_eval(emu, ts, tape, soa)
    assert res.ok, res.why
    bad = [r for r in range(len(want)) if res.values[r] != want[r]]
    assert not bad, (tag, bad[:4], hex(res.values[bad[0]]), hex(want[bad[0]]))
    return legacy_entries(emu), res.dyn["f64"], res.dyn["valu"]


@pytest.mark.parametrize("div", list(wc.DIVISORS))
def test_rows_meet_every_case(cases, div):
    """The C oracle alone: the crafted rows of each shape satisfy x = q y + r, and between them
    put each of the digits 0, 1, 2^31, 2^32 - 1 at every position, reach the 2^32 clamp, leave a
    remainder with limb j + ny nonzero, and hold x < y, x = y and (variable shapes) y = 0, y = 1
    and a short divisor; the signed rows have dividends of both signs and -2^255."""
    ts, idx = cases
    how, p = wc.DIVISORS[div]
    for xn, bits in wc.DIVIDENDS.items():
        tq, tr = idx["%s_%s_udiv_v" % (xn, div)][0], idx["%s_%s_urem_v" % (xn, div)][0]
        cr = wc.crafted(11, div, xn, False)
        labels = {c[0] for c in cr}
        digits, clamp, borrow = set(), False, False
        ny = wc.declared_ny(div, False)
        for label, xr, yr, short in cr:
            xm, ym = xr & ((1 << bits) - 1), wc.eff_y(div, yr)
            q, r = ctape.evaluate(ts, tq, [xr, yr, 0]), ctape.evaluate(ts, tr, [xr, yr, 0])
            if ym == 0:
                assert (q, r) == (wc.M, xm), label
                continue
            assert xm == q * ym + r and r < ym, label
            assert short == (wc.limbs(ym) < ny), label
            if not short and ny <= 7 and bits // 32 >= ny:
                d, c_, b_ = wc.digit_facts(xm, ym, ny)
                digits |= d
                clamp |= c_
                borrow |= b_
        assert {"x < y", "x = 0"} <= labels
        if how != "const":
            assert {"y = 1", "y = 0"} <= labels
            assert (ny > 1) == ("short divisor" in labels)
        if ny <= 7 and bits // 32 >= ny:
            j0 = bits // 32 - ny
            if how != "const" or j0 > 0:
                assert clamp and (borrow or ny == 1 or j0 == 0), (div, xn, clamp, borrow)
            for j in range(j0):     # every position below the top one holds all four digits
                assert {(j, d) for d in wc.DIGITS} <= digits, (div, xn, j)
            assert any(pos == j0 for pos, _ in digits) or how == "const", (div, xn)
    sg = wc.crafted(11, div, "x", True)
    assert any(c[1] >> 255 for c in sg) and any(not c[1] >> 255 for c in sg)
    assert any(c[1] == 1 << 255 for c in sg)


@pytest.mark.parametrize("div", list(wc.DIVISORS))
def test_values_and_paths(emu, monkeypatch, cases, div):
    """Per shape and kind, values and Bool tape: the oracle's values on every row at every
    level; at level 5 a variant site's hot waves never enter the legacy code and run fewer f64
    ops than at level 4, and each wave with a short-divisor lane enters it once."""
    ts, idx = cases
    for xn in wc.DIVIDENDS:
        sets = {}
        for signed in (False, True):
            ws = wc.waves(21, div, xn, signed)
            hot, _ = wc.flatten([w for w in ws if w[0] == wc.HOT])
            short = [r for w in ws if w[0] == wc.SHORT for r in w[1]]
            sets[signed] = (hot, short, sum(1 for w in ws if w[0] == wc.SHORT))
        for op, _ in wc.OPS:
            hot, short, n_short = sets[wc.is_signed(div, xn, op)]
            is_var = wc.variant(div, xn, op)
            for form in ("v", "b"):
                name = "%s_%s_%s_%s" % (xn, div, op, form)
                tape = idx[name][0]
                soa_h, want_h = soa_of(hot, ts.n_vars), [ctape.evaluate(ts, tape, r) for r in hot]
                got = {}
                for cfg in CONFIGS:
                    configure(monkeypatch, *cfg)
                    got[cfg] = run(emu, ts, tape, soa_h, want_h, (name, cfg))
                if is_var:
                    assert got[("5", None)][0] == 0 and got[(None, None)][0] == 0, (name, got)
                    assert got[("4", None)][0] > 0, (name, got)
                    # one limb under a full-width dividend runs the same eight digits and the
                    # same Newton steps as L_NARROW: what goes is the OR tree and the borrow
                    # chain, integer work; every other shape drops f64 ops
                    same_f64 = wc.declared_ny(div, wc.is_signed(div, xn, op)) == 1 and \
                        xn == "x" and wc.DIVISORS[div][0] != "const"
                    if same_f64:
                        assert got[("5", None)][1] == got[("4", None)][1], (name, got)
                    else:
                        assert got[("5", None)][1] < got[("4", None)][1], (name, got)
                    assert got[("5", None)][2] < got[("4", None)][2], (name, got)
                if short:
                    soa_s = soa_of(short, ts.n_vars)
                    want_s = [ctape.evaluate(ts, tape, r) for r in short]
                    for cfg in (("4", None), ("5", None)):
                        configure(monkeypatch, *cfg)
                        n = run(emu, ts, tape, soa_s, want_s, (name, cfg, "short"))[0]
                        if is_var:
                            assert n == n_short, (name, cfg, n, n_short)


def test_constant_divisors_declare_zero_limbs(emu, monkeypatch, cases):
    """udiv / urem by a nonzero constant: the limbs the site declares zero (quotient limbs above
    nx - ny, remainder limbs from ny up) are zero in the oracle's value on every row, and the
    emitted code, which stores them as constants, agrees."""
    ts, idx = cases
    configure(monkeypatch, "5", None)
    for div in ("c32", "c160", "c224"):
        ny = wc.declared_ny(div, False)
        for xn, bits in wc.DIVIDENDS.items():
            if bits // 32 < ny:
                continue
            rows, _ = wc.flatten(wc.waves(31, div, xn, False)[:6])
            soa = soa_of(rows, ts.n_vars)
            for op, top in (("udiv", 32 * (bits // 32 - ny + 1)), ("urem", 32 * ny)):
                tape = idx["%s_%s_%s_v" % (xn, div, op)][0]
                want = [ctape.evaluate(ts, tape, r) for r in rows]
                assert all(v >> top == 0 for v in want), (div, xn, op)
                run(emu, ts, tape, soa, want, (div, xn, op))


def test_level_4_keeps_the_parent_build(monkeypatch):
    configure(monkeypatch, "4", None)
    assert native.jit_code_id(synth.generate()) == "04a963fc0464aa45"


def test_module_without_variant_site_keeps_its_text(emu, monkeypatch):
    """The dispatch and the variants are printed only into a module one of whose tapes calls
    one: full-width divisions give the same text at levels 4 and 5, a short divisor does not."""
    def module(short):
        ts = TapeSet()
        b = ts.builder()
        x, y = b.var("x"), b.var("y")
        yy = b.op(Op.ZEXT, b.op(Op.EXTRACT, y, imm0=159, imm1=0), imm0=96) if short else y
        ts.add(b.finish(b.op(Op.BVUREM, x, yy)))
        ts.add(b.finish(b.op(Op.BVSMOD, b.op(Op.BVADD, x, y), y)))
        return ts

    text = {}
    for short in (False, True):
        for level in ("4", "5"):
            configure(monkeypatch, level, None)
            text[short, level] = jit_module(emu, module(short), assemble=False)[0]
    assert text[False, "4"] == text[False, "5"]
    assert "mh_dv_L128:" not in text[False, "5"] and "mh_dv_L128:" not in text[True, "4"]
    assert "mh_dv_L128:" in text[True, "5"] and "mh_dv_L129:" in text[True, "5"]
    # legacy part of the routine: the same lines in the same order
    legacy = text[True, "4"][text[True, "4"].index("mh_dv_L1:"):].split("s_setpc_b64")[0]
    assert legacy in text[True, "5"]


def test_config5_levels_agree(emu, monkeypatch):
    """Config-5 tapes 0-299 x 128 generated rows: identical values at levels 4 and 5, with
    fewer f64 ops executed at level 5."""
    ts = synth.generate(300)
    seed = synth.load_spec()["assignment_seed"]
    soa = soa_of([smt_eval.gen_assignment(seed, ts.n_vars, r) for r in range(128)], ts.n_vars)
    vals, f64 = {}, {}
    for level in ("4", "5"):
        configure(monkeypatch, level, None)
        res = [jit_eval(emu, ts, i, soa) for i in range(len(ts.tapes))]
        vals[level] = [r.values for r in res]
        f64[level] = sum(r.dyn["f64"] for r in res if r.ok)
    assert vals["4"] == vals["5"]
    assert sum(v is not None for v in vals["5"]) >= 290
    print("f64 ops executed", f64)
    assert f64["5"] < f64["4"], f64
