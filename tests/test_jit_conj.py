"""Random root conjunctions (tests/conj_cases.py) through the tape JIT's count path on the host
wave emulator: every tape at MH_JIT_STAGE 0, 1, 2 and unset and once without the short circuit,
every root bit of every row against the C oracle.  Beside the parity, each seed must show that
the staged path was really taken: tapes jitted, code that differs from level 0, rows that hit and
rows that miss, waves the slice decided and waves that fell back to the full cone."""
import random

import pytest

from tests import conj_cases as cc
from tests.emu import jit_eval, set_short_circuit

LEVELS = ("0", "1", "2", None)


def n_cols_of(seed):
    return 4 if seed % 2 == 0 else 7


def jit_any_budget(emu, ts, tape, soa):
    """jit_eval at 128 VGPRs, then at 168 (mh_tapes_jit's retry)."""
    res = jit_eval(emu, ts, tape, soa)
    return res if res.ok else jit_eval(emu, ts, tape, soa, max_vgpr=168)


def run_tape(emu, monkeypatch, ts, tape, rows, soa):
    """{level: JitResult} of a jitted tape (None if refused at level 0), every build checked
    against the oracle on every row."""
    want = None
    out = {}
    for level in LEVELS:
        if level is None:
            monkeypatch.delenv("MH_JIT_STAGE", raising=False)
        else:
            monkeypatch.setenv("MH_JIT_STAGE", level)
        builds = [(level, True)] + ([(level, False)] if level is None else [])
        for lv, short_circuit in builds:
            set_short_circuit(emu, short_circuit)
            try:
                res = jit_any_budget(emu, ts, tape, soa)
            finally:
                set_short_circuit(emu, True)
            if not res.ok:
                if short_circuit:
                    out[lv] = None
                continue
            if want is None:
                want = cc.root_bits(ts, tape, rows).tolist()
            bad = [r for r in range(len(rows)) if res.values[r] != want[r]]
            assert not bad, (lv, short_circuit, tape, bad[:4], [hex(v) for v in rows[bad[0]]])
            if short_circuit:
                out[lv] = res
    return out, want


def is_staged(out):
    a, b = out["0"], out[None]
    return (a.code_bytes, a.n_valu) != (b.code_bytes, b.n_valu)


@pytest.mark.parametrize("seed", range(8))
def test_random_conjunctions(emu, monkeypatch, seed):
    ts, rows = cc.random_set(seed, n_cols_of(seed))
    assert len(ts.tapes) == cc.N_TAPES and len(rows) % 64
    soa = cc.soa_of(rows, ts.n_vars)
    refused = staged = mixed = decided = fell_back = 0
    for t in range(len(ts.tapes)):
        out, want = run_tape(emu, monkeypatch, ts, t, rows, soa)
        if any(out[lv] is None for lv in LEVELS):
            refused += 1
            continue
        mixed += 0 < sum(want) < len(rows)
        if is_staged(out):
            staged += 1
            decided += out[None].dyn["valu"] < out["0"].dyn["valu"]
            fell_back += out[None].dyn["valu"] > out["0"].dyn["valu"]
    print("random seed %d: %d cols, %d rows, jitted %d, staged %d, mixed %d, slice decided %d, "
          "fallback ran %d" % (seed, ts.n_vars, len(rows), cc.N_TAPES - refused, staged, mixed,
                               decided, fell_back))
    assert refused <= 2
    assert staged >= 8
    assert mixed >= 8
    assert decided >= 1 and fell_back >= 1


@pytest.mark.parametrize("seed", range(8))
def test_near_ties(emu, monkeypatch, seed):
    """Each conjunction on a wave per (d7, sign of lo) pair crafted for it, the near-tie lane
    alone among 63 random rows, and on the row set the GPU test uploads (every pair once per set,
    dealt over the conjunctions)."""
    ts, triples, set_rows, _ = cc.near_tie_case(seed, n_cols_of(seed))
    set_soa = cc.soa_of(set_rows, ts.n_vars)
    staged = 0
    for i, tr in enumerate(triples):
        rows = cc.near_tie_rows(ts, tr, random.Random(1000 * seed + i))
        assert len(rows) == 64 * len(cc.TIE_PAIRS)
        out, _ = run_tape(emu, monkeypatch, ts, tr[0], rows, cc.soa_of(rows, ts.n_vars))
        assert all(out[lv] is not None for lv in LEVELS), (seed, tr[0])
        staged += is_staged(out)
        run_tape(emu, monkeypatch, ts, tr[0], set_rows, set_soa)
    print("near-tie seed %d: %d cols, %d rows in the set, jitted %d, staged %d"
          % (seed, ts.n_vars, len(set_rows), len(triples), staged))
    assert staged >= 3
