"""Open top-limb products of the tape JIT (jit.cpp op_mul_open, MH_JIT_STAGE=4) on the host wave
emulator: the tapes and rows of tests/mul_open_cases.py at levels 3, 4 and unset and once without
the short circuit, every root against the C oracle; the executed multiply-adds of decided and
undecided waves; the slack bound itself, in Python integers; and the level-3 build id."""
import ctypes as C
import os
import random
import re

import pytest

from mythril_amd import native, synth
from tests import conj_cases as cc
from tests import mul_open_cases as mc
from tests.emu import jit_eval, jit_module, set_short_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL3_BUILD = "84f13e6e7f455321"   # config-5 code id before the open products
LEVELS = ("3", "4", None)


def _enum(path, head):
    src = open(os.path.join(ROOT, "mythril_amd", "csrc", path)).read()
    body = src[src.index(head):]
    body = re.sub(r"//[^\n]*", "", body[body.index("{") + 1:body.index("};")])
    names, nxt = {}, 0
    for ent in [e.strip() for e in body.split(",") if e.strip()]:
        if "=" in ent:
            ent, val = [s.strip() for s in ent.split("=")]
            nxt = int(val, 0) if val[0].isdigit() else names[val]
        names[ent] = nxt
        nxt += 1
    return names


D_MUL_R = _enum("dev_isa.h", "enum mh_dop")["D_MUL_R"]
M_V_MAD_U64_U32 = _enum("jit.h", "enum Op : uint16_t")["M_V_MAD_U64_U32"]


def mul_mads(emu, reset=True):
    """Executed v_mad_u64_u32 emitted by D_MUL_R since the last reset."""
    f = emu.lib.emu_jit_tag_op
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    buf = (C.c_uint64 * (256 * 128))()
    f(buf, int(reset))
    return int(buf[128 * D_MUL_R + (M_V_MAD_U64_U32 & 127)])


def set_level(monkeypatch, level):
    if level is None:
        monkeypatch.delenv("MH_JIT_STAGE", raising=False)
    else:
        monkeypatch.setenv("MH_JIT_STAGE", level)


def check_tape(emu, monkeypatch, ts, tape, rows):
    """{level: JitResult}: every build's roots equal the C oracle's on every row."""
    soa = cc.soa_of(rows, ts.n_vars)
    want = cc.root_bits(ts, tape, rows).tolist()
    out = {}
    for level in LEVELS + ("full",):
        set_level(monkeypatch, None if level == "full" else level)
        set_short_circuit(emu, level != "full")
        try:
            res = jit_eval(emu, ts, tape, soa)
        finally:
            set_short_circuit(emu, True)
        assert res.ok, (level, tape, res.why)
        bad = [r for r in range(len(rows)) if res.values[r] != want[r]]
        assert not bad, (level, tape, bad[:4], [hex(v) for v in rows[bad[0]]])
        out[level] = res
    return out, want


@pytest.fixture(scope="module", params=[4, 7])
def built(request):
    ts, cases = mc.build(request.param)
    return request.param, ts, cases


def test_roots_match_the_oracle(emu, monkeypatch, built):
    n_cols, ts, cases = built
    opened = 0
    for case in cases:
        rows, at = mc.case_rows(case, n_cols)
        assert len(rows) % 64 == 0 and len(at) >= 20
        out, want = check_tape(emu, monkeypatch, ts, case.tape, rows)
        a, b = out["3"], out["4"]
        differs = (a.code_bytes, a.n_valu) != (b.code_bytes, b.n_valu)
        opened += differs
        assert (out[None].code_bytes, out[None].n_valu) == (b.code_bytes, b.n_valu)
        if case.name == "c_k0":
            continue     # x * 0: there is no product
        assert 0 < sum(want) < len(rows), case.name
        if case.name == "cutoff_sum":
            # past the D > 64 cut-off the conjunct is unstaged: level 0's code
            monkeypatch.setenv("MH_JIT_STAGE", "0")
            z = jit_eval(emu, ts, case.tape, cc.soa_of(rows[:64], ts.n_vars))
            assert (z.code_bytes, z.n_valu) == (b.code_bytes, b.n_valu)
        else:
            assert differs, case.name
    assert opened >= len(cases) - 2


def test_exact_products_keep_level_3_text(emu, monkeypatch, built):
    n_cols = built[0]
    ts, names = mc.build_exact(n_cols)
    monkeypatch.setenv("MH_JIT_STAGE", "3")
    t3, _, n3 = jit_module(emu, ts, assemble=False)
    monkeypatch.setenv("MH_JIT_STAGE", "4")
    t4, _, n4 = jit_module(emu, ts, assemble=False)
    assert n3 == n4 == len(names)
    assert t3 == t4
    rng = random.Random(5)
    rows = mc.decidable_rows(rng, n_cols, 64)
    for t in range(len(names)):
        check_tape(emu, monkeypatch, ts, t, rows)


def test_executed_multiply_adds(emu, monkeypatch, built):
    """A wave of decided rows runs the two top columns of an open product, at most 15
    multiply-adds; one undecided live lane makes the wave run the full product as well."""
    n_cols, ts, cases = built
    by_name = {c.name: c for c in cases}
    rng = random.Random(77)
    for name in ("vv_ult", "vv_sge", "sq", "c_kfull", "c_k32", "chain_add_sub"):
        case = by_name[name]
        decided = mc.decidable_rows(rng, n_cols, 64)
        p, q = rng.getrandbits(256), rng.getrandbits(256)
        tie = mc.crafted_rows(case, (p, q), n_cols, points="few")[0]   # R's top limb on T
        undecided = [list(r) for r in decided]
        undecided[29] = [v if i in mc.LAYOUT[n_cols] else undecided[29][i]
                         for i, v in enumerate(tie)]
        got = {}
        for level in ("0", "4"):
            monkeypatch.setenv("MH_JIT_STAGE", level)
            for tag, rows in (("decided", decided), ("undecided", undecided)):
                mul_mads(emu)
                res = jit_eval(emu, ts, case.tape, cc.soa_of(rows, ts.n_vars))
                assert res.ok
                got[level, tag] = mul_mads(emu)
        full = got["0", "decided"]       # the plain code runs the product once, in full
        assert full == got["0", "undecided"]
        assert 0 < got["4", "decided"] <= 15 and got["4", "decided"] < full, (name, got)
        assert got["4", "undecided"] == got["4", "decided"] + full, (name, got)
        if name.startswith("vv") or name == "sq":
            assert full == 36 and got["4", "decided"] == 15, (name, got)


def patterns():
    """(name, limb kinds of a, limb kinds of b, draw a, draw b) of every product of the cases."""
    def var(rng):
        r = rng.random()
        if r < 0.5:
            return rng.getrandbits(256)
        if r < 0.8:
            return sum(rng.choice([0, 1, mc.M32, mc.M32 - 1, rng.getrandbits(32)]) << (32 * k)
                       for k in range(8))
        return mc.M - rng.getrandbits(rng.choice([1, 8, 40, 200]))

    out = [("vv", mc.VAR, mc.VAR, var, var)]
    for name, k in mc.CONSTS + [("kodd", mc.K_ODD)]:
        out.append((name, mc.VAR, mc.limbs(k), var, lambda rng, k=k: k))
    return out


def test_slack_bound_property():
    """0 <= limb7(a b) - T (mod 2^32) <= hi over 10^5 operand pairs and the extremes, under each
    constant-limb pattern of the cases; hi from the Python restatement of the emitter's rule."""
    rng = random.Random(0xB0D)
    pats = patterns()
    assert mc.open_hi(mc.VAR, mc.VAR) == 6
    assert mc.open_hi(mc.VAR, mc.limbs(1)) == 0 and mc.open_hi(mc.VAR, mc.limbs(0)) == 0
    assert mc.open_hi(mc.VAR, mc.limbs(0xDEADBEEF)) == 1
    n = 0
    worst = {}
    for name, ka, kb, da, db in pats:
        hi = mc.open_hi(ka, kb)
        assert hi <= 7
        extremes = [(mc.M, mc.M), (0, 0), (1, 1), (mc.M, 1), (mc.M - 1, mc.M),
                    (mc.LOW, mc.LOW), (mc.M ^ mc.M32, mc.M)]
        draws = 100000 // len(pats) + 1
        for i in range(draws + len(extremes)):
            a, b = extremes[i - draws] if i >= draws else (da(rng), db(rng))
            if kb is not mc.VAR:
                b = db(rng)
            if name == "vv" and i % 7 == 0:
                b = a                                    # x * x
            e = mc.open_e(a, b)
            assert e <= hi, (name, hex(a), hex(b), e, hi)
            worst[name] = max(worst.get(name, 0), e)
            n += 1
    assert n >= 100000
    assert worst["vv"] >= 5      # the draws reach the top of the range, not just its middle


def test_level_3_is_the_build_before(monkeypatch):
    """MH_JIT_STAGE=3 emits the code of the build before the open products, text for text."""
    monkeypatch.setenv("MH_JIT_STAGE", "3")
    assert native.jit_code_id(synth.generate()) == LEVEL3_BUILD
