"""Level-6 entries of the division subroutine (jit.cpp op_div / div_routine, MH_JIT_STAGE=6: the
raw srem entry and the run-time width dispatch) on the host wave emulator, whose v_rcp_f32 and
v_rcp_f64 are the approximate ones.

Every tape of tests/div_entry_cases.py gives the C oracle's value on every row at MH_JIT_STAGE 5,
6 and unset and with MH_JIT_DIV=0.  The emulator's counters say which code ran at level 6: the
sites call exactly as often as at level 5; a wave all of whose lanes the raw srem entry decides
never enters the legacy code (label L_UNS), a wave with an undecided lane enters it once; a wave
whose divisors all have the same run-time width enters that width's variant, a wave with one lane
of another width, or a zero divisor, does not.  Level 5 keeps the parent's build id, and a module
that does not divide keeps its text."""
import ctypes as C

import pytest

from mythril_amd import native, synth
from mythril_amd.tape import Op, TapeSet
from oracle import ctape
from tests import div_entry_cases as ec
from tests.emu import jit_eval, jit_module
from tests.test_jit import soa_of

L_UNS, L_SRAW, L_SCOLD, L_BGO = 1, 113, 114, 116
# (MH_JIT_STAGE, MH_JIT_DIV)
CONFIGS = (("5", None), ("6", None), (None, None), (None, "0"))


@pytest.fixture(scope="module")
def cases():
    return ec.build()


def configure(monkeypatch, stage, div):
    monkeypatch.delenv("MH_JIT_ENTRY", raising=False)
    for name, v in (("MH_JIT_STAGE", stage), ("MH_JIT_DIV", div)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def counters(emu, name, n):
    f = getattr(emu.lib, name)
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    h = (C.c_uint64 * n)()
    f(h, 1)
    return [int(v) for v in h]


def run(emu, ts, tape, rows, want, tag):
    """(calls, label counts) of the tape over the rows, after checking every value."""
    counters(emu, "emu_jit_div_hist", 32)
    counters(emu, "emu_jit_div_labels", 128)
    res = jit_eval(emu, ts, tape, soa_of(rows, ts.n_vars))
    assert res.ok, res.why
    bad = [r for r in range(len(want)) if res.values[r] != want[r]]
    assert not bad, (tag, bad[:4], hex(res.values[bad[0]]), hex(want[bad[0]]))
    return sum(counters(emu, "emu_jit_div_hist", 32)), counters(emu, "emu_jit_div_labels", 128)


def by_kind(waves):
    """{kind: (rows, number of waves)}, each set closed by a partial copy of its first wave."""
    out = {}
    for kind in {w[0] for w in waves}:
        rows, kinds = ec.flatten([w for w in waves if w[0] == kind])
        out[kind] = (rows, len(kinds))
    return out


def test_rows_meet_every_case():
    """The oracle alone: the crafted lanes hold what their labels say."""
    cr = ec.crafted_a(11)
    labels = {c[0] for c in cr}
    for want in ("signs 00", "signs 01", "signs 10", "signs 11", "x = -2^255, y = 1",
                 "x = -2^255, y = -1", "x = -2^255, y = -2^255", "|x| < |y|", "c = 1",
                 "c = 2^10 - 1", "c = 2^10", "x = 77 y", "short y", "y = 0", "borrow through",
                 "m != 0, P = 0", "c = 40, thr above", "c = 40, thr below"):
        assert want in labels, want
    sgn = lambda v: v - (1 << 256) if v >> 255 else v
    for label, x, y, kind in cr:
        if y == 0:
            continue
        c, frac = divmod(abs(sgn(x)), abs(sgn(y)))
        if kind == ec.HOT:
            assert c < 1 << 10 and abs(sgn(y)) - 1 >> 224, label
            assert c == 0 or 0 < frac, label
        if label.startswith("x = ") and label.endswith(" y"):
            assert frac == 0 and c == int(label.split()[2]), label
        if label == "m != 0, P = 0":
            assert c == 0 and (x ^ y) >> 255, label
    assert {k for *_, k in cr} == {ec.HOT, ec.COLD, ec.EDGE}
    for kind, rows, ny, label in ec.waves_b(12):
        tops = {max(((r[1] >> r[3] if r[3] < 256 else 0).bit_length() + 31) // 32, 0) for r in rows}
        assert (tops == {ny}) == (kind == ec.DISPATCH), (label, tops)


@pytest.mark.parametrize("name", ec.A_TAPES)
def test_raw_srem_values_and_paths(emu, monkeypatch, cases, name):
    ts, idx = cases
    tape = idx[name]
    sites = 2 if name == "srem_urem_v" else 1
    for kind, (rows, n_waves) in by_kind(ec.waves_a(21)).items():
        want = [ctape.evaluate(ts, tape, r) for r in rows]
        got = {}
        for cfg in CONFIGS:
            configure(monkeypatch, *cfg)
            got[cfg] = run(emu, ts, tape, rows, want, (name, kind, cfg))
        calls5, lab5 = got[("5", None)]
        for cfg in (("6", None), (None, None)):
            calls6, lab6 = got[cfg]
            assert calls6 == calls5 == sites * n_waves, (name, kind, cfg, calls6, calls5)
            assert lab6[L_SRAW] == n_waves, (name, kind, lab6[L_SRAW])
            # the urem site of the two-site tape is a legacy call at either level
            legacy = lab6[L_UNS] - (sites - 1) * n_waves
            if kind == ec.HOT:
                assert legacy == 0 and lab6[L_SCOLD] == 0, (name, cfg, legacy)
            elif kind == ec.COLD:
                assert legacy == n_waves and lab6[L_SCOLD] == n_waves, (name, cfg, legacy)
            else:
                assert legacy == lab6[L_SCOLD] <= n_waves, (name, cfg, legacy)
        assert lab5[L_SRAW] == 0 and lab5[L_UNS] == sites * n_waves, (name, kind)


@pytest.mark.parametrize("name", ec.B_TAPES)
def test_width_dispatch_values_and_paths(emu, monkeypatch, cases, name):
    ts, idx = cases
    tape = idx[name]
    waves = ec.waves_b(22)
    for kind in (ec.DISPATCH, ec.LEGACY):
        for ny in sorted({w[2] for w in waves if w[0] == kind}):
            rows, kinds = ec.flatten([w for w in waves if w[0] == kind and w[2] == ny])
            n_waves = len(kinds)
            want = [ctape.evaluate(ts, tape, r) for r in rows]
            got = {}
            for cfg in CONFIGS:
                configure(monkeypatch, *cfg)
                got[cfg] = run(emu, ts, tape, rows, want, (name, kind, ny, cfg))
            calls5, lab5 = got[("5", None)]
            assert sum(lab5[L_BGO + 1:L_BGO + 7]) == 0
            for cfg in (("6", None), (None, None)):
                calls6, lab6 = got[cfg]
                assert calls6 == calls5 == n_waves, (name, kind, ny, calls6, calls5)
                assert lab6[L_UNS] == n_waves, (name, kind, ny, lab6[L_UNS])
                entered = sum(lab6[L_BGO + 1:L_BGO + 7])
                if kind == ec.DISPATCH:
                    assert lab6[L_BGO + ny - 1] == entered == n_waves, (name, ny, entered)
                else:
                    assert entered == 0, (name, ny, entered)


def test_one_layer_at_a_time(emu, monkeypatch, cases):
    """MH_JIT_ENTRY builds one layer alone (scripts/div_entry_stats.py prices them so): with the
    raw srem entry only, its fallback into the legacy code is not dispatched; with the dispatch
    only, no call takes the raw entry."""
    ts, idx = cases
    rows, kinds = ec.flatten([w for w in ec.waves_b(22) if w[0] == ec.DISPATCH and w[2] == 5])
    for name in ("w_srem_v", "wn_srem_v"):
        want = [ctape.evaluate(ts, idx[name], r) for r in rows]
        for entry, raw, dispatched in (("1", len(kinds), 0), ("2", 0, len(kinds)),
                                       ("3", len(kinds), len(kinds))):
            configure(monkeypatch, "6", None)
            monkeypatch.setenv("MH_JIT_ENTRY", entry)
            calls, lab = run(emu, ts, idx[name], rows, want, (name, entry))
            assert calls == len(kinds)
            assert lab[L_SRAW] == raw and lab[L_SCOLD] == raw, (name, entry, lab[L_SRAW])
            assert sum(lab[L_BGO + 1:L_BGO + 7]) == dispatched, (name, entry)


def test_level_5_keeps_the_parent_build(monkeypatch):
    configure(monkeypatch, "5", None)
    assert native.jit_code_id(synth.generate()) == "5014909b621f244c"


def test_module_text_by_level(emu, monkeypatch):
    """A module that does not divide has the same text at levels 5 and 6; one that divides prints
    the new entries at level 6 only, and its level-5 text has none of their labels."""
    def module(divides):
        ts = TapeSet()
        b = ts.builder()
        x, y = b.var("x"), b.var("y")
        ts.add(b.finish(b.op(Op.BVSREM if divides else Op.BVMUL, x, y)))
        ts.add(b.finish(b.op(Op.BVADD, x, y)))
        return ts

    text = {}
    for divides in (False, True):
        for level in ("5", "6"):
            configure(monkeypatch, level, None)
            text[divides, level] = jit_module(emu, module(divides), assemble=False)[0]
    assert text[False, "5"] == text[False, "6"]
    assert "mh_div:" not in text[False, "6"]
    for lbl in ("mh_dv_L113:", "mh_dv_L114:", "mh_dv_L115:", "mh_dv_L123:"):
        assert lbl in text[True, "6"] and lbl not in text[True, "5"], lbl
    assert "mh_dv_L128:" in text[True, "6"] and "mh_dv_L128:" not in text[True, "5"]
    legacy = text[True, "5"][text[True, "5"].index("mh_dv_L1:"):].split("s_setpc_b64")[0]
    assert "mh_dv_L1:" in text[True, "6"] and len(legacy) < len(text[True, "6"])
